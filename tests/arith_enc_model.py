"""What the tests of arith_dynamic encoding share (test_arith_enc_cpu.py, test_gpu_arith_enc.py): the model's encoder
(arith_model.py: M.Encoder, M.encode_core, M.compress - pinned to the reference's streams by test_arith_cpu.py) wrapped so
that it counts the range coder's output events and says which candidate streams arith_compress_to codes, and the lists of
inputs the GPU tests encode.  arith_model.py is not edited: the wrapper stands in for M.Encoder while a core coder runs.
Everything is seeded; nothing here needs a GPU.

Events, keyed (home, event) with home "o0" / "o1_lds" / "o1_global" as on the device:
  carry            a symbol's low wrapped (Carry set)
  ff_pending       a shift that only counts a pending 0xFF byte (FFNum)
  ff_flush_plain   pending bytes written without a carry (as 0xFF)
  ff_flush_carry   pending bytes written behind a carry (as 0x00)
  ff_run2          two or more pending bytes written at once
  shift2           two shifts in one symbol
  ff_at_finish     bytes still pending when the coder finishes
  ended_early      the device's early end: the alphabet byte, the bytes written and the bytes pending reach the input's
                   length before the last symbol is coded (the reference then stores the bytes, arith_dynamic.c:850)"""
import collections
import functools
import random

import arith_cases as K
import arith_model as M

KINDS = ("o0", "o1_lds", "o1_global", "rle", "stored")
EVENTS = ("carry", "ff_pending", "ff_flush_plain", "ff_flush_carry", "ff_run2", "shift2", "ff_at_finish", "ended_early")


class CountingEncoder(M.Encoder):
    def __init__(self, n, events, home):
        super().__init__()
        self.n, self.ev, self.home = n, events, home
        self.shifts = 0
        self.early = n <= 1                                  # before the first symbol: the alphabet byte alone

    def _count(self, what):
        if self.ev is not None:
            self.ev[self.home, what] += 1

    def _shift_low(self):
        self.shifts += 1
        if self.low < 0xff000000 or self.carry:
            if self.ffnum:
                self._count("ff_flush_carry" if self.carry else "ff_flush_plain")
                if self.ffnum >= 2:
                    self._count("ff_run2")
        else:
            self._count("ff_pending")
        super()._shift_low()

    def symbol(self, m, sym):
        self.shifts = 0
        i = m.S.index(sym)
        if (self.low + sum(m.F[:i]) * (self.range // m.tot)) > M.M32:
            self._count("carry")
        super().symbol(m, sym)
        assert self.shifts <= 2
        if self.shifts == 2:
            self._count("shift2")
        if not self.early and 1 + len(self.out) + self.ffnum >= self.n:
            self.early = True

    def finish(self):
        if self.ffnum:
            self._count("ff_at_finish")
        return super().finish()


def encode_core(data, order1, rle, events=None, home="o0"):
    """M.encode_core(data, order1, rle) with the events counted: (body, ended early).  A stream the early end cuts
    counts the events of the whole stream all the same: the census is of the inputs, the device codes a prefix."""
    made = []

    def factory():
        made.append(CountingEncoder(len(data), events, home))
        return made[0]
    keep, M.Encoder = M.Encoder, factory
    try:
        body = M.encode_core(data, order1, rle)
    finally:
        M.Encoder = keep
    early = made[0].early
    assert not early or len(body) >= len(data)               # what ends early is stored
    if early and events is not None:
        events[home, "ended_early"] += 1
    return body, early


def home_of(order1, m):
    return "o0" if not order1 else "o1_lds" if M.lds_home(m) else "o1_global"


def _plain(data, order, trace, events):
    """M.compress for an order word without X_STRIPE, restated with its candidate traced (test_arith_enc_cpu.py holds it to
    M.compress)"""
    n = len(data)
    flags = order & 0xff
    meta = b"" if flags & M.X_NOSZ else M.var_put(n)
    order &= 3
    if flags & M.X_PACK and n:
        pmeta, packed = M.hts_pack(data)
        if len(pmeta) == 1 and pmeta[0] > 16:
            flags &= ~M.X_PACK
        else:
            data, n = packed, len(packed)
            meta += pmeta + M.var_put(n)
    elif flags & M.X_PACK:
        flags &= ~M.X_PACK
    if flags & M.X_RLE and not n:
        flags &= ~M.X_RLE
    if order and n < 8:
        flags &= ~3
        order = 0
    assert not flags & M.X_EXT
    cand = {"flags": flags, "n": n, "stored": True, "coded": False}
    if not flags & M.X_CAT:
        m = (max(data) if data else 0) + 1
        cand.update(coded=True, home=home_of(order == 1, m), rle=bool(flags & M.X_RLE), m=m)
        body, early = encode_core(data, order == 1, bool(flags & M.X_RLE), events, cand["home"])
        cand.update(stored=len(body) >= n, early=early, body=len(body))
    if cand["stored"]:
        flags = (flags & ~(3 | M.X_EXT)) | M.X_CAT
        body = data
    if trace is not None:
        trace.append(cand)
    return bytes([flags]) + meta + body


def compress(data, order, trace=None, events=None):
    """M.compress(data, order); trace: a list that takes every candidate stream (a dict: coded, home, rle, stored, early,
    n, body), a stripe block's planes under each of their methods; events: a Counter for the census"""
    data = bytes(data)
    n = len(data)
    if n <= 20:
        order &= ~M.X_STRIPE
    if not order & M.X_STRIPE:
        return _plain(data, order, trace, events)
    N = (order >> 8) or 4
    assert N <= 255
    head = bytes([order & 0xff & ~M.X_NOSZ]) + M.var_put(n) + bytes([N])
    lens, body = b"", b""
    for i in range(N):
        best = None
        for meth in M.STRIPE_METHODS[min(i, 3)]:
            if (order & 3) == 0 and (meth & 1):
                continue
            c = _plain(data[i::N], meth | M.X_NOSZ, trace, events)
            if best is None or len(c) < len(best):
                best = c
        lens += M.var_put(len(best))
        body += best
    return head + lens + body


def route_of(trace):
    """the route read-out (R4X16_ROUTE_ARITH_ENC) of the candidates in `trace`"""
    r = dict.fromkeys(KINDS, 0)
    for c in trace:
        if c["coded"]:
            r[c["home"]] += 1
            r["rle"] += c["rle"]
        r["stored"] += c["stored"]
    return r


def refused(size, order):
    """the status of a block the order word alone refuses (0: none)"""
    if order & M.X_STRIPE and size > 20:
        return M.E_UNSUPPORTED if ((order >> 8) or 4) > 255 else 0
    return M.E_UNSUPPORTED if order & M.X_EXT else 0


# ---- the lists the GPU tests encode ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_cases():
    """[(file name, text, order, the reference's stream)]"""
    return [(fn, M.text(base), order, s) for fn, base, order, s in M.fixtures()]


@functools.lru_cache(maxsize=None)
def edge_cases():
    """[(what, data, order, the reference's stream)] of tests/golden/arith/edge.bin"""
    return [(what, data, order, s) for what, order, data, s in K.edge()[0]]


def shifted(name, by, n=None):
    """a golden text with every byte raised: an alphabet above 84, whose order-1 rows take the global home"""
    t = M.text(name)[:n]
    return bytes((c + by) & 0xff for c in t)


def all_pairs(m):
    """every pair of symbols below m exactly once (a de Bruijn sequence of order 2): each order-1 context meets a symbol it
    has not seen every time it is used, which costs more than eight bits from the fourteenth use on - the one way to an
    early end with an alphabet that fits the LDS home"""
    out, a = [], [0] * (2 * m)

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                out.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, m):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(out)


def packed_planes():
    """128 bytes in eight planes of 16: the first two of bytes that no coder shortens, the others of 16 symbols each -
    packed they halve, behind a map of 17 bytes and a length"""
    rng = random.Random(3)
    planes = [bytes(rng.sample(range(256), 16)) for _ in range(2)] + [bytes(rng.sample(range(7 * j, 7 * j + 16), 16)) for j in range(6)]
    return bytes(planes[i % 8][i // 8] for i in range(128))


def _search(rng, want, tries=200000):
    """short inputs of 2 - 4 symbols, drawn until want(data) holds"""
    for _ in range(tries):
        k = rng.randrange(2, 5)
        syms = rng.sample(range(256), k)
        data = bytes(rng.choice(syms) for _ in range(rng.randrange(8, 40)))
        if want(data):
            return data
    raise AssertionError("no such input")


@functools.lru_cache(maxsize=None)
def boundary_cases():
    """[(what, data, order)]: per home (order 0; order 1 with a low and a high alphabet) inputs whose coded size is one
    below their length (coded), their length and one above it (ended early and stored), twice each"""
    out = []
    for home, order, lo in (("o0", 0, 0), ("o1_lds", 1, 0), ("o1_global", 1, 100)):
        rng = random.Random(len(home) * 7 + order)
        for d in (-1, 0, 1):
            for rep in range(2):
                def want(data):
                    if order and M.lds_home(max(data) + 1) != (lo == 0):
                        return False
                    return len(M.encode_core(data, order, False)) == len(data) + d
                out.append(("%s coded size n%+d" % (home, d), _search(rng, want), order))
    return out


@functools.lru_cache(maxsize=None)
def step_cases():
    """[(what, data, order)]: arith_cases' inputs that drive the model's step - the climber across every lane boundary,
    alphabets of every size, skewed symbols with runs - in each home, with and without run lengths (its halving ties,
    K.tie_cases(), are a list of their own: the model takes seconds over them)"""
    out = []
    for m in (5, 64, 65, 200, 256):
        out += [("climber m=%d" % m, K.climber(m, 2 * m + 20), o) for o in (0, 1, 64, 65)]
    for m in (1, 2, 3, 4, 5, 63, 64, 65, 84, 85, 128, 255, 256):
        out += [("m=%d" % m, K.with_alphabet(m, 300 + m % 16, m), o) for o in (0, 1, 64, 65)]
    for k, (lo, hi) in enumerate(((40, 72), (30, 84), (120, 250))):
        for o in (0, 1, 64, 65, 128 + 65):
            for n in range(700, 700 + (16, 16, 40)[k]):
                out.append(("skewed %d..%d n=%d" % (lo, hi, n), K.skewed(tuple(range(lo, hi, 3)), n, 50 + k, runs=5), o))
    out += [("all pairs m=%d" % m, all_pairs(m), o) for m in (80, 84, 120) for o in (1, 65)]
    out.append(("ties", K.ties(200), 0))
    out.append(("ties", K.ties(200), 1))
    # the global home at a text's length: carries and pending bytes by the thousand
    out += [("q4 + 100", shifted("q4", 100, 40000), 1), ("q4 + 100", shifted("q4", 100, 40000), 65)]
    return out


@functools.lru_cache(maxsize=None)
def rare_cases():
    """[(what, data, order)]: seeded searches for the events no list above reaches twice in a home - bytes pending at the
    finish, runs of pending bytes - one search an event and a home"""
    out = []
    for home, order, lo in (("o0", 0, 0), ("o1_lds", 1, 0), ("o1_global", 1, 100)):
        for what in ("ff_at_finish", "ff_run2"):
            rng = random.Random(len(home) * 31 + len(what))
            for rep in range(2):
                def want(data):
                    if order and M.lds_home(max(data) + 1) != (lo == 0):
                        return False
                    ev = collections.Counter()
                    body, _ = encode_core(data, order, False, ev, home)
                    return ev[home, what] > 0
                out.append(("%s %s" % (home, what), _search(rng, want), order))
    return out


@functools.lru_cache(maxsize=None)
def trip_cases():
    """1,100 inputs of 200 bytes with an alphabet above 84 under order 1: more items of the global home than it has slots"""
    return [("global trip %d" % i, K.skewed(tuple(range(90 + i % 50, 250, 7)), 200, 3000 + i), 1) for i in range(1100)]
