"""tests/golden/tok3/edge.bin - reference-made tok3 containers of small name blocks, one per branch and side
(README.edge.md beside it; oracle/make_tok3_edge.py made it with oracle/_ref/tok3_ref) - and the seeded random name
blocks the tok3 edge tests share with that script.

  cases()                         every case of the fixture: .name, .block, .vectors = [(level, use_arith, last_start, container)]
  names_of(block, last_start)     what decode_names gives for a block: every line end a NUL
  random_block(rng, ..)           one random block of a kind
  random_blocks(seed, count, ..)  a seeded list of them

Test infrastructure only: nothing in htscodecs_amd/ imports this module."""
import collections
import functools
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = os.path.join(ROOT, "tests", "golden", "tok3", "edge.bin")
README = os.path.join(ROOT, "tests", "golden", "tok3", "README.edge.md")
MAGIC = b"TOK3EDG1\n"

Case = collections.namedtuple("Case", "name block vectors")
Vector = collections.namedtuple("Vector", "level use_arith last_start container")


def write(path, cases):
    out = bytearray(MAGIC + len(cases).to_bytes(4, "little"))
    for c in cases:
        name = c.name.encode()
        out += len(name).to_bytes(2, "little") + name
        out += len(c.block).to_bytes(4, "little") + c.block
        out += len(c.vectors).to_bytes(4, "little")
        for v in c.vectors:
            out += v.level.to_bytes(4, "little") + v.use_arith.to_bytes(4, "little") + v.last_start.to_bytes(4, "little")
            out += len(v.container).to_bytes(4, "little") + v.container
    with open(path, "wb") as f:
        f.write(out)


@functools.lru_cache(maxsize=None)
def cases():
    with open(EDGE, "rb") as f:
        buf = f.read()
    assert buf[:len(MAGIC)] == MAGIC
    at = len(MAGIC)

    def u(n):
        nonlocal at
        at += n
        return int.from_bytes(buf[at - n:at], "little")

    def take(n):
        nonlocal at
        at += n
        assert at <= len(buf)
        return bytes(buf[at - n:at])

    out = []
    for _ in range(u(4)):
        name = take(u(2)).decode()
        block = take(u(4))
        vectors = []
        for _ in range(u(4)):
            level, use_arith, last_start = u(4), u(4), u(4)
            vectors.append(Vector(level, use_arith, last_start, take(u(4))))
        out.append(Case(name, block, tuple(vectors)))
    assert at == len(buf)
    return tuple(out)


def vectors(use_arith=None, level=None):
    """[(case, vector)] of a flavour and a level (None: any), in the fixture's order."""
    return [(c, v) for c in cases() for v in c.vectors
            if (use_arith is None or v.use_arith == use_arith) and (level is None or v.level == level)]


def names_of(block, last_start):
    return bytes(0 if ch <= 10 else ch for ch in block[:last_start])


# ---- random blocks -------------------------------------------------------------------------------------------------
# 13 small alphabets: few symbols, so that names share prefixes, repeat, and put every byte class beside every other
ALPHABETS = (b"ab", b"ab:_9", b"0123", b"a0:. ", b"Az09:_-/#@> ", b"a1", b"09", b"a:", b"x0 ", b"abc019._",
             b"\x0b\x1f\x7f a0", b"@>m_/-:f0", b"Zz!~0189")
SEPARATORS = (b"\n", b"\0", b"\x01", b"\n\0\x01")
PLAIN, LONG, DUPS = "plain", "long", "dups"


def random_block(rng, kind=PLAIN, max_names=150, max_len=100):
    """PLAIN: 1 .. max_names names of up to max_len bytes (and up to 10 more where a number is spliced in) drawn from a
    pool of names over one alphabet, mutated, cut short, with 9- and 10-digit numbers spliced in; LONG: the same with
    names of 65 .. 120 single-byte tokens among them (N_END at 66 .. 121: the tokeniser's second pass); DUPS: 300 .. 400
    names from a pool of 10.  Separators are '\\n', NUL and 0x01; one block in five ends in an unterminated tail.  No
    name reaches 127 tokens, no byte is >= 0x80, and every block holds a terminated name."""
    alpha = rng.choice(ALPHABETS)
    seps = rng.choice(SEPARATORS)
    word = lambda n: bytes(rng.choice(alpha) for _ in range(n))
    if kind == DUPS:
        pool = [word(rng.randrange(0, 12)) for _ in range(10)]
        names = [rng.choice(pool) for _ in range(rng.randrange(300, 401))]
    else:
        pool = [word(rng.randrange(0, max_len + 1)) for _ in range(40)]
        names = []
        for _ in range(rng.randrange(1, max_names + 1)):
            n = bytearray(rng.choice(pool))
            if n and rng.random() < 0.5:
                n[rng.randrange(len(n))] = rng.choice(alpha)
            if rng.random() < 0.2:
                del n[rng.randrange(len(n) + 1):]
            if rng.random() < 0.15:
                at = rng.randrange(len(n) + 1)
                n[at:at] = b"%d" % rng.randrange(10 ** 8, 10 ** 10)
            names.append(bytes(n))
        if kind == LONG:
            letters, digits = rng.choice((b"ab", b"x", b" -")), rng.choice((b"0123", b"19", b"0"))
            tall = [bytes(rng.choice(letters if k % 2 == 0 else digits) for k in range(rng.randrange(65, 121))) for _ in range(3)]
            for _ in range(rng.randrange(2, 8)):
                n = bytearray(rng.choice(tall))
                if rng.random() < 0.6:
                    k = rng.randrange(len(n))
                    n[k] = rng.choice(letters if k % 2 == 0 else digits)
                names.insert(rng.randrange(len(names) + 1), bytes(n))
    block = b"".join(n + bytes([rng.choice(seps)]) for n in names)
    if rng.random() < 0.2:
        block += word(rng.randrange(1, 12))
    return block


def random_blocks(seed, count, kinds=(PLAIN,), **kw):
    """count blocks, kinds[k % len(kinds)] for the k-th."""
    rng = random.Random(seed)
    return [random_block(rng, kinds[k % len(kinds)], **kw) for k in range(count)]
