#!/usr/bin/env python3
"""Make tests/golden/rans/edge.bin and the tables of README.edge.md: small inputs, one per branch of the reference's rANS
4x16 and 4x8 encoders and side of it, with the streams the REFERENCE wrote for them, and 600 damaged streams a codec with
the reference's answer to each (oracle/_ref/rans_ref: the reference's unchanged sources behind oracle/rans_ref_driver.c,
sanitizers on; `make -C oracle` builds it where a reference tree is).

Nothing of this project's oracle, library or kernels has a say in what is written: the inputs and the damage are made
here, the answers are the driver's.  An encode case is kept only where the reference ran clean and decoded its own stream
back to the input; every case below is expected to be kept, and the script exits non-zero if one is not.  Where a case
is "the last input on one side of a test and the first on the other", the reference's own streams say which inputs
those are (their flag byte, their header), out of a family of inputs made here.

A damaged stream is run twice (tests/rans_edge_cases.py, RUN_A and RUN_B: stack paint, earlier call, heap fill); equal
answers make it stable and it is stored with the answer - refused, or length and SHA-256 - different ones, or a report,
make it unstable and it is stored without.

The script also sends every entry of tests/golden/edge.json (oracle-made, oracle/make_golden.py) through the driver and
writes into the README how many of them the reference reproduces by length and MD5; all, or it exits non-zero.

    python oracle/make_rans_edge.py            write the fixture and rewrite the README's tables between their markers
    python oracle/make_rans_edge.py --check    make everything again and compare with what is committed
"""
import collections
import hashlib
import json
import os
import random
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import datagen
import rans_edge_cases as X

BEGIN, END = "<!-- table: begin (oracle/make_rans_edge.py) -->", "<!-- table: end -->"
BEGIN2, END2 = "<!-- counts: begin (oracle/make_rans_edge.py) -->", "<!-- counts: end -->"
PLAIN = (0, 1, 64, 65, 128, 129, 192, 193)
STRIPE = X.X_STRIPE
SEED, PER_CODEC = 20261021, 600
SKEW_256 = [40 if i % 16 == 0 else 1 for i in range(256)]       # all 256 byte values, skewed enough for order 0 to pay
# cases whose branch lies in a table, an alphabet or a transform: a stream that fell back to a plain X_CAT copy (no
# transform flag kept) would not hold it
NO_CAT = ("pack_", "rle_", "o1_alphabet_run_", "o1table_", "o1shift_", "norm_one", "norm_total", "norm_largest", "large_", "stripe_methods_")


def text(n, seed=1, alphabet=b"FFFFFFFF:::,,#<-"):
    rng = random.Random(seed)
    return bytes(rng.choice(alphabet) for _ in range(n))


def no_runs(n, seed=1, nsym=200):
    """n bytes without two equal neighbours."""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        c = rng.randrange(nsym)
        if not out or out[-1] != c:
            out.append(c)
    return bytes(out)


def flags_of(stream):
    return stream[0]


def rle_meta_raw(stream):
    """The low bit of the RLE meta size of a plain X_RLE stream with a size field: 1 = meta stored raw (:1304)."""
    at = 1 + X.varint(stream, 1)[1]
    return X.varint(stream, at)[0] & 1


def o1_head(stream):
    leaf = X.leaves16(stream)[0]
    return None if leaf["at"] is None or not leaf["order"] else leaf["src"][leaf["at"]]


def tie_planes():
    """Two interleaved copies of the shortest plane, out of a family made here, for which the reference's X_RLE | X_NOSZ
    stream keeps its X_RLE flag and is as long as its X_NOSZ stream of order 0."""
    planes = [b"".join(bytes([65 + i * 7 % 3]) * (1 + i * 5 % 4 + (i % 9 == 0) * k % 7) for i in range(k))[:k] for k in range(24, 424)]
    res = X.run_driver([(X.OP_C16, flags, 0, 0, p) for p in planes for flags in (0x50, 0x10)])
    for p, a, b in zip(planes, res[0::2], res[1::2]):
        if a[0] == b[0] == X.MADE and len(a[2]) == len(b[2]) and a[2][0] & X.X_RLE and len(a[2]) < len(p):
            return bytes(c for pair in zip(p, p) for c in pair)
    raise AssertionError("no plane of the family ties")


# ---- the encode cases ------------------------------------------------------------------------------------------------
def candidates():
    """[(name, branch, side, codec, spec or bytes, orders)]; which members of a family are kept is pick_families' to say."""
    out = []
    add = lambda name, branch, side, codec, data, orders: out.append((name, branch, side, codec, data, tuple(orders)))

    # size and header
    for n in range(34):
        side = {0: "no input", 20: "the last size at which X_STRIPE is dropped", 21: "the first striped size"}.get(n, "%d bytes" % n)
        add("size_%02d" % n, "size and header (:1151, :1322, :1332)", side, 16, text(n, 3), PLAIN + (8, 9, 16, 17, 32, 33))
    # stripe
    for N in (2, 3, 4, 5, 8, 32):
        for r in range(N):
            n = (96 if N == 32 else 40) // N * N + r
            add("stripe_%d_r%d" % (N, r), "X_STRIPE part lengths (:1168-1180)", "N = %d, in_size %% N = %d" % (N, r), 16, text(n, 5 + N), (N << 8 | 8,))
    add("stripe_default_n", "X_STRIPE N (:1155-1156)", "N = 0, read as 4", 16, text(45, 6), (8, 9, 0xc9))
    for methods in (0, 1, 64, 128, 193):
        side = "methods {%s}" % ", ".join(str(m) for m in (1, 64, 128) if methods & m == m and m) if methods else "methods {0}"
        add("stripe_methods_%d" % methods, "X_STRIPE method pick (:1190-1211)", side + " and 0", 16,
            ["runs", 900, 4, 9, 2, 48] if methods else text(400, 8), (4 << 8 | 8 | methods, 3 << 8 | 8 | methods))
    add("stripe_tie", "X_STRIPE method pick (:1199)", "planes of 6 bytes: every method falls back to X_CAT at one size, the first tried stands", 16,
        text(24, 9), (4 << 8 | 8 | 193,))
    add("stripe_tie_rle", "X_STRIPE method pick (:1199)", "two equal planes on which X_RLE and plain order 0 give streams of one size and other bytes: "
        "X_RLE, tried first, stands (best_sz > olen2 is strict)", 16, tie_planes(), (2 << 8 | 8 | 64,))
    # PACK
    for nsym in (1, 2, 3, 4, 5, 16, 17, 256):
        side = {1: "1 symbol: no payload", 17: "17 symbols: refused, pmeta_len == 1 and out[c_meta_len] > 16",
                256: "256 symbols: hts_pack gives its one meta byte 0, which is not > 16"}.get(nsym, "%d symbols" % nsym)
        add("pack_%d" % nsym, "X_PACK (:1244-1267)", side, 16, bytes(range(256)) + datagen.weighted(3800, SKEW_256, 7).tobytes() if nsym == 256 else ["rand", 67, 7, nsym, 40], (128, 129, 192, 193))
    for per, nsym in ((8, 2), (4, 4), (2, 16)):
        for r in range(per):
            add("pack_%dper_r%d" % (per, r), "X_PACK lengths (pack.c:56-151)", "%d symbols a byte, length %% %d = %d" % (per, per, r), 16,
                ["rand", 64 + r, 11, nsym, 65], (128,))
    for n, left in ((56, 7), (57, 8), (64, 8)):
        add("pack_o1_left_%d_%d" % (left, n), "order bit cleared below 8 bytes (:1322)", "%d bytes of 2 symbols pack to %d: order 1 %s" % (n, left, "dropped" if left < 8 else "kept"), 16,
            ["rand", n, 12, 2, 65], (129,))
    # RLE
    for run in (255, 256, 257):
        add("rle_run_%d" % run, "X_RLE run lengths (rle.c:48-187)", "a run of %d" % run, 16, b"ab" * 20 + b"c" * run + b"ba" * 20, (64, 65))
    add("rle_run_70000", "X_RLE run lengths (rle.c:48-187)", "a run of 70,000", 16, ["const", 70000, 67], (64, 65, 192))
    add("rle_all_symbols", "X_RLE run symbols (:1277-1285)", "all 256 symbols as run symbols (meta byte 0)", 16, bytes(s for s in range(256) for _ in range(4)), (64, 65))
    for m in range(1, 40):                                        # every run of three saves one byte: the sums step by one, equality included
        add("rle99_%02d" % m, "X_RLE worth it: rle_len + rmeta_len >= .99 * in_size (:1287)", "family: 1,000 bytes, %d runs of 3 of one symbol" % m, 16,
            b"".join(b"\xfa\xfa\xfa" + bytes([201 + k % 40]) for k in range(m)) + no_runs(1000 - 4 * m, 13), (64,))
    for k in range(1, 41):
        add("rlemeta_%02d" % k, "X_RLE meta compressed or raw (:1299)", "family: %d bytes of runs over 2 symbols" % (50 * k), 16,
            ["runs", 50 * k, 2, 4, 20, 48], (64,))
    # CAT
    add("cat_explicit", "X_CAT asked for (:1218-1225)", "with a size field and with X_NOSZ", 16, text(300, 14), (32, 33, 48, 49))
    for n in range(10, 90):
        add("catfall_%02d" % n, "X_CAT as fall-back (:1332)", "family: %d bytes of text" % n, 16, text(n, 15), (0, 16))
    # order-1 tables
    for nsym in (2, 3, 256):
        add("o1_alphabet_run_%d" % nsym, "alphabet run shortcut (:225-255)", "%d consecutive symbols" % nsym, 16,
            ["weighted", 60000, SKEW_256, 16] if nsym == 256 else ["rand", 300, 16, nsym, 65], (1, 0))
    for nsym in (4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 64):
        add("o1table_%02d" % nsym, "order-1 table compressed or raw (:735-760)", "family: 3,000 bytes over %d symbols" % nsym, 16, ["markov", 3000, nsym, 17, 33, 0.55], (1,))
    for k, w in enumerate((2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 1024, 3000)):
        add("o1shift_%02d" % k, "compute_shift: 10 or 12 bits (:620-691)", "family: 60,000 bytes, one symbol %d times as likely as each of 255 others" % w, 16,
            ["weighted", 60000, [w] + [1] * 255, 18], (1,))
    # normalise_freq
    add("norm_one_symbol", "normalise_freq (:141-199)", "one symbol", 16, ["const", 1000, 65], (0, 1))
    add("norm_256_once", "normalise_freq (:141-199)", "256 symbols once each", 16, bytes(range(256)), (0, 1))
    for n in (1023, 1024, 1025, 4095, 4096, 4097):
        add("norm_total_%d" % n, "normalise_freq and the shift / round2 path (:141-199, :535)", "a total of %d over 5 symbols" % n, 16, ["rand", n, 19, 5, 65], (0,))
    add("norm_largest_corrects", "normalise_freq (:141-199)", "200 symbols once or twice and one 3,700 times: the largest frequency takes the whole correction", 16,
        ["weighted", 4099, [3000] + [1] * 200, 20], (0, 1))
    # large, kept as length and SHA-256
    add("large_rand", "a large input", "70,000 bytes over 256 symbols", 16, ["weighted", 70000, SKEW_256, 21], (0, 1, 193))
    add("large_text", "a large input", "65,536 bytes of quality text", 16, ["tile", "q40+dir", 65536, 0, 0], (0, 1, 193, 4 << 8 | 0xc9))

    # 4x8
    for n in range(1, 10):
        add("x8_size_%d" % n, "4x8 size (rANS_static.c:438: order 1 below 4 bytes is order 0)", "%d bytes" % n, 8, text(n, 22), (0, 1))
    for nsym in (1, 2, 255, 256):
        add("x8_alphabet_%d" % nsym, "4x8 alphabet", "%d symbols" % nsym, 8, ["rand", 3000 if nsym > 2 else 200, 23, nsym, 0 if nsym > 2 else 65], (0, 1))
    for run in (2, 3):
        add("x8_symbol_run_%d" % run, "4x8 symbol run shortcut (:143-169)", "%d consecutive symbols" % run, 8, ["rand", 200, 24, run, 65], (0, 1))
    add("x8_freq_127", "4x8 frequency forms (:160-166)", "a frequency of 127: one byte", 8, (b"A" + b"B" * 32) * 3 + b"A" + b"B" * 29, (0,))
    add("x8_freq_128", "4x8 frequency forms (:160-166)", "a frequency of 128: two bytes", 8, (b"A" + b"B" * 31) * 4, (0,))
    add("x8_large", "a large input", "70,000 bytes of quality text", 8, ["tile", "q8", 70000, 0, 0], (0, 1))
    return out


def pick_families(made):
    """made: {name: [stream per order]} of the candidates the reference encoded and decoded back.  The names of family
    members that are NOT kept, and {name: side} for the kept ones.  A family is ordered; a neighbouring pair on either
    side of the reference's own decision is kept."""
    drop, sides = set(), {}

    def family(prefix, decide, words, every=False):
        names = sorted(n for n in made if n.startswith(prefix))
        got = [(n, decide(made[n][0])) for n in names]
        pairs = [(a, b) for a, b in zip(got, got[1:]) if a[1] != b[1]]
        assert pairs, (prefix, got)
        keep = {}
        for a, b in (pairs if every else pairs[:1]):
            keep[a[0]] = "the last of the family with %s" % words[a[1]]
            keep[b[0]] = "the first with %s" % words[b[1]]
        for n in names:
            if n in keep:
                sides[n] = keep[n]
            else:
                drop.add(n)

    family("rle99_", lambda s: bool(s[0] & X.X_RLE), {True: "X_RLE kept", False: "X_RLE dropped"})
    family("rlemeta_", lambda s: (bool(s[0] & X.X_RLE), rle_meta_raw(s) if s[0] & X.X_RLE else None),
           collections.defaultdict(lambda: "X_RLE dropped", {(True, 0): "the meta compressed", (True, 1): "the meta raw"}), every=True)
    family("catfall_", lambda s: bool(s[0] & X.X_CAT), {True: "X_CAT (not compressed)", False: "an order-0 payload"})
    other = lambda words: collections.defaultdict(lambda: "no order-1 payload", words)
    family("o1table_", lambda s: None if o1_head(s) is None else o1_head(s) & 1, other({0: "the table raw", 1: "the table compressed"}), every=True)
    family("o1shift_", lambda s: None if o1_head(s) is None else o1_head(s) >> 4, other({10: "a shift of 10", 12: "a shift of 12"}), every=True)
    return drop, sides


def input_of(data):
    return datagen.make(data).tobytes() if isinstance(data, list) else bytes(data)


def make_cases():
    todo = candidates()
    assert len({t[0] for t in todo}) == len(todo)
    enc, index = [], []
    for k, (name, _, _, codec, data, orders) in enumerate(todo):
        raw = input_of(data)
        for o in orders:
            enc.append((X.OP_C16 if codec == 16 else X.OP_C8, o, 0, 0, raw))
            index.append((k, o))
    res = X.run_driver(enc)
    dec = []
    for (k, o), (answer, _, stream), rec in zip(index, res, enc):
        codec = todo[k][3]
        if answer != X.MADE:
            dec.append(None)
        elif codec == 8:
            dec.append((X.OP_U8, 0, 0, 0, stream))
        else:
            dec.append((X.OP_U16_TO, len(rec[4]), 0, 0, stream))
    back = iter(X.run_driver([d for d in dec if d is not None]))
    made, lost = collections.defaultdict(list), []
    for (k, o), (answer, value, stream), rec, d in zip(index, res, enc, dec):
        name = todo[k][0]
        if d is None:
            lost.append((name, o, "refused" if answer == X.REFUSED else "report %#x" % value))
            continue
        b = next(back)
        if b[0] != X.MADE or b[2] != rec[4]:
            lost.append((name, o, "the reference did not decode its own stream back"))
            continue
        made[name].append(stream)
    orders_of = {t[0]: t[5] for t in todo}
    drop, sides = pick_families({n: s for n, s in made.items() if len(s) == len(orders_of[n])})
    cases, rows = [], []
    for name, branch, side, codec, data, orders in todo:
        if name in drop:
            continue
        if len(made.get(name, ())) != len(orders):
            continue
        raw = input_of(data)
        large = len(raw) > 4099
        if name.startswith(NO_CAT) and name not in sides:
            for o, st in zip(orders, made[name]):
                if st[0] & X.X_CAT and not st[0] & (X.X_STRIPE | X.X_PACK | X.X_RLE):
                    lost.append((name, o, "the reference's stream is an X_CAT copy: the case does not reach its branch"))
        if name.startswith(("o1_alphabet_run_256", "pack_256")):
            assert len(set(raw)) == 256, name
        assert isinstance(data, list) or not large
        vectors = tuple(X.Vector(o, X.digest(s) if large else s) for o, s in zip(orders, made[name]))
        spec = json.dumps(data) if isinstance(data, list) else ""
        cases.append(X.Case(name, codec, spec, X.digest(raw) if spec else raw, vectors))
        rows.append("| `%s` | %s | %s | %d | %s |" % (name, branch, "%s; %s" % (side, sides[name]) if name in sides else side, len(raw),
                                                ", ".join("%#x: %d" % (o, len(s)) for o, s in zip(orders, made[name]))))
    lost = [l for l in lost if l[0] not in drop]
    table = ["| case | branch | side | bytes | order: length of the reference's stream |", "|---|---|---|---|---|"] + rows
    return cases, "\n".join(table) + "\n", lost


# ---- inputs that are no vectors ------------------------------------------------------------------------------------------
def no_vectors():
    """The inputs the README lists as no vectors, each shown again: [(what, how the reference answers)]."""
    big = datagen.make(["rand", 16384, 41, 256, 0]).tobytes()
    recs = [(X.OP_C16, 1 << 8 | 8, 0, 0, big), (X.OP_C16, 255 << 8 | 8, 0, 0, text(131, 42)), (X.OP_C16, 32 << 8 | 8, 0, 0, text(21, 43)), (X.OP_C8, 0, 0, 0, b"")]
    res = X.run_driver(recs)
    back = X.run_driver([(X.OP_U16_TO, len(big), 0, 0, res[0][2])])[0]
    assert res[0][0] == X.MADE and (back[0] != X.MADE or back[2] != big)
    assert all(r[0] == X.REPORT for r in res[1:]), res[1:]
    say = lambda r: "a sanitizer report" if r[1] & 0x100 else "signal %d" % r[1]
    return [("X_STRIPE with N = 1 over 16,384 bytes", "a stream the reference does not decode back (%s)" % ("refused" if back[0] == X.REFUSED else "other bytes" if back[0] == X.MADE else say(back))),
            ("X_STRIPE with N = 255 over 131 bytes", say(res[1])), ("X_STRIPE with N = 32 over 21 bytes (in_size < N)", say(res[2])),
            ("rans_compress (4x8) over 0 bytes", say(res[3]))]


# ---- the old vectors ---------------------------------------------------------------------------------------------------
def old_vectors():
    with open(os.path.join(ROOT, "tests", "golden", "edge.json")) as f:
        old = json.load(f)["cases"]
    res = X.run_driver([(X.OP_C16, e["order"], 0, 0, datagen.make(e["in"]).tobytes()) for e in old])
    same = sum(r[0] == X.MADE and len(r[2]) == e["len"] and hashlib.md5(r[2]).hexdigest() == e["md5"] for r, e in zip(res, old))
    return same, len(old)


# ---- damaged streams -------------------------------------------------------------------------------------------------
def crafted(codec, bases_by_kind):
    """Streams put together here from reference-made parts, for the deviations the draw does not reach:
    [(codec, stream, op, capacity)]."""
    out = []
    if codec == 8:
        # a 4x8 order-0 table of two symbols, listed in descending order
        data, s = bases_by_kind["x8_two_symbols"]
        a = s[9]
        at = 10 + (2 if s[10] >= 128 else 1)
        b = s[at]
        assert a + 1 < b
        out.append((8, s[:9] + bytes([b]) + s[10:at] + bytes([a]) + s[at + 1:], X.OP_U8, 0))
        # an order-1 stream one of whose initial states points at slot 4095 of context 0's 4095-sum table: of the four
        # states of three reference-made streams, the first the reference answers stably and accepts
        tries = []
        for kind in ("x8_order1_a", "x8_order1_b", "x8_order1_c"):
            data, s = bases_by_kind[kind]
            t = X.tables8(s)
            assert t["order"] == 1 and t["rows"][0] == (0, 0, 4095)
            for k in range(4):
                at = t["end"] + 4 * k
                tries.append(s[:at] + b"\xff" + bytes([s[at + 1] | 0x0f]) + s[at + 2:])
        answers = X.answers_ab([(X.OP_U8, 0, b) for b in tries])
        good = [b for b, a in zip(tries, answers) if a is not None and a != X.REFUSED]
        assert good, "no state of the three streams gives a stable accepted answer"
        out.append((8, good[0], X.OP_U8, 0))
        return out
    # a stripe stream as the one plane of a stripe stream
    data, inner = bases_by_kind["stripe"]
    out.append((16, bytes([STRIPE]) + varint_bytes(len(data)) + b"\x01" + varint_bytes(len(inner)) + inner, X.OP_U16, 0))
    # an order-1 table sent as an order-0 stream of 204,801 bytes: the raw table, then zeros
    data, s = bases_by_kind["o1_raw_table"]
    leaf = X.leaves16(s)[0]
    at = leaf["at"]
    table_len = o1_raw_table_len(s, at)
    padded = s[at + 1:at + 1 + table_len] + bytes(204801 - table_len)
    packed = X.run_driver([(X.OP_C16, X.X_NOSZ, 0, 0, padded)])[0]
    assert packed[0] == X.MADE and packed[2][0] == X.X_NOSZ
    nested = packed[2][1:]
    out.append((16, s[:at] + bytes([s[at] | 1]) + varint_bytes(len(padded)) + varint_bytes(len(nested)) + nested + s[at + 1 + table_len:], X.OP_U16, 0))
    # a stripe stream of two planes: a reference-made order-1 stream, and the same stream with the row of one context
    # (one that the plane's data uses) resent as all zeros, so that the second plane has no row for it
    data, s = bases_by_kind["o1_plane"]
    leaf = X.leaves16(s, len(data))[0]
    assert s[0] == X.X_NOSZ | 1 and leaf["at"] is not None
    shift, compressed, _, rows, spans = X.o1_table(s, leaf["at"])
    assert not compressed and rows and all(rows.values())
    ctx = max(c for c in rows if bytes([c]) in data[:-1])
    first, end = spans[ctx]
    second = s[:first] + b"\0" + bytes([len(rows) - 1]) + s[end:]
    out.append((16, bytes([STRIPE]) + varint_bytes(2 * len(data)) + b"\x02" + varint_bytes(len(s)) + varint_bytes(len(second)) + s + second, X.OP_U16, 0))
    return out


def varint_bytes(v):
    out = [v & 0x7f]
    v >>= 7
    while v:
        out.append(0x80 | v & 0x7f)
        v >>= 7
    return bytes(reversed(out))


def o1_raw_table_len(s, at):
    """Bytes of the raw order-1 table behind the header byte s[at], read as X.o1_table reads it."""
    lo, hi = 1, len(s) - at - 17
    want = X.o1_table(s, at)[3]
    assert want
    while lo < hi:                               # the shortest prefix that reads the same rows (ends early -> None)
        mid = (lo + hi) // 2
        if X.o1_table(s[:at + 1 + mid], at)[3] == want:
            hi = mid
        else:
            lo = mid + 1
    return lo


def make_damaged():
    rng = random.Random(SEED)
    bases, damaged = [], []
    counts = {}
    for codec in (16, 8):
        # base streams: reference-made, 30 .. 1,500 bytes
        recs = []
        while len(recs) < 400:
            data = X.random_input(rng, 1200)
            if codec == 8:
                if data:
                    recs.append((X.OP_C8, rng.randrange(2), 0, 0, data))
            else:
                recs.append((X.OP_C16, X.random_order(rng), 0, 0, data))
        special = []
        if codec == 16:
            special = [("stripe", (X.OP_C16, 2 << 8 | 8 | 1, 0, 0, text(120, 31))), ("o1_raw_table", (X.OP_C16, 1, 0, 0, text(400, 32, b"ACGT"))),
                       ("o1_plane", (X.OP_C16, X.X_NOSZ | 1, 0, 0, text(300, 34, b"ACGT")))]
        else:
            special = [("x8_two_symbols", (X.OP_C8, 0, 0, 0, text(200, 33, b"AAAC")))]
            special += [("x8_order1_" + k, (X.OP_C8, 1, 0, 0, text(n, seed, b"AAACGT"))) for k, n, seed in (("a", 120, 35), ("b", 200, 36), ("c", 300, 37))]
        res = X.run_driver(recs + [r for _, r in special])
        by_kind = {k: (r[4], a[2]) for (k, r), a in zip(special, res[len(recs):])}
        good = [(r, a[2]) for r, a in zip(recs, res) if a[0] == X.MADE and 30 <= len(a[2]) <= 1500]
        good.sort(key=lambda g: len(g[1]))
        good = good[:len(good) * 2 // 3]                          # the shorter two thirds: the fixture stays small
        if codec == 16:                                           # 12 stripe streams, 12 without a size field, 36 others
            kind = lambda s: 0 if s[0] & STRIPE else 1 if s[0] & X.X_NOSZ else 2
            picked = [g for k, n in ((0, 12), (1, 12), (2, 36)) for g in rng.sample([g for g in good if kind(g[1]) == k], n)]
        else:
            picked = rng.sample(good, 60)
        extra = crafted(codec, by_kind)
        first = len(bases)
        calls, meta = [], []
        per = (PER_CODEC - len(extra)) // len(picked)
        spare = PER_CODEC - len(extra) - per * len(picked)
        for k, (rec, s) in enumerate(picked):
            bases.append((codec, s))
            for _ in range(per + (k < spare)):
                edits = tuple(X.damage(rng, s, codec))
                b = X.apply(s, edits)
                if codec == 8:
                    op, cap = X.OP_U8, 0
                elif s[0] & X.X_NOSZ and not s[0] & STRIPE or rng.random() < 0.5:
                    op, cap = X.OP_U16_TO, len(rec[4]) + rng.choice((0, 0, 64))
                else:
                    op, cap = X.OP_U16, 0
                calls.append((op, cap, b))
                meta.append((first + k, op, cap, edits))
        for c, s, op, cap in extra:
            bases.append((c, s))
            calls.append((op, cap, s))
            meta.append((len(bases) - 1, op, cap, ()))
        assert len(calls) == PER_CODEC
        answers = X.answers_ab(calls)
        for (base, op, cap, edits), a in zip(meta, answers):
            damaged.append(X.Damaged(base, op, cap, edits, None if a is None else X.REFUSED if a == X.REFUSED else X.digest(a)))
        stable = sum(a is not None for a in answers)
        accepted = sum(a is not None and a != X.REFUSED for a in answers)
        assert stable >= 400 and accepted >= 100, (codec, stable, accepted)
        members = {d.name: sum(bool(d.predicate(b, cap)) and a is not None and a != X.REFUSED for (_, cap, b), a in zip(calls, answers))
                   for d in X.DEVIATIONS if d.codec == codec and d.what == "decode"}
        counts[codec] = (stable, accepted, PER_CODEC - stable, members)
    return tuple(bases), tuple(damaged), counts


def make():
    cases, table, lost = make_cases()
    same, total = old_vectors()
    bases, damaged, counts = make_damaged()
    lines = ["* `tests/golden/edge.json`: the reference reproduces %d of its %d entries by length and MD5." % (same, total)]
    for codec in (16, 8):
        stable, accepted, unstable, members = counts[codec]
        lines.append("* rANS 4x%d: %d damaged streams, %d stable (%d accepted, %d refused), %d unstable." % (codec, PER_CODEC, stable, accepted, stable - accepted, unstable))
        for name, n in members.items():
            lines.append("  * `%s`: its predicate holds for %d streams that the reference accepts stably." % (name, n))
    for what, how in no_vectors():
        lines.append("* no vector: %s: %s." % (what, how))
    if same != total:
        lost.append(("edge.json", 0, "%d of %d entries not reproduced" % (total - same, total)))
    return X.Fixture(tuple(cases), bases, damaged), table, "\n".join(lines) + "\n", lost


def between(text_, begin, end, new):
    head, rest = text_.split(begin)
    return head + begin + "\n" + new + end + rest.split(end, 1)[1]


def main():
    if not os.path.exists(X.DRIVER):
        sys.exit("no %s: make -C oracle builds it where a reference tree is" % X.DRIVER)
    fx, table, counts, lost = make()
    for name, order, why in lost:
        print("NOT KEPT: %s under %#x: %s" % (name, order, why))
    with open(X.README) as f:
        text_ = f.read()
    new = between(between(text_, BEGIN, END, table), BEGIN2, END2, counts)
    if "--check" in sys.argv[1:]:
        fd, tmp = tempfile.mkstemp()
        os.close(fd)
        X.write(tmp, fx)
        with open(tmp, "rb") as f, open(X.EDGE, "rb") as g:
            same = f.read() == g.read()
        os.unlink(tmp)
        print("fixture %s, tables %s" % ("same" if same else "DIFFERS", "same" if new == text_ else "DIFFERS"))
        sys.exit(1 if lost or not same or new != text_ else 0)
    X.write(X.EDGE, fx)
    with open(X.README, "w") as f:
        f.write(new)
    print("%d cases, %d vectors, %d base streams, %d damaged, %d bytes" % (len(fx.cases), sum(len(c.vectors) for c in fx.cases), len(fx.bases), len(fx.damaged),
                                                                         os.path.getsize(X.EDGE)))
    print(counts, end="")
    sys.exit(1 if lost else 0)


if __name__ == "__main__":
    main()
