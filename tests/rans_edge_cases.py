"""tests/golden/rans/edge.bin - reference-made rANS 4x16 and 4x8 streams of small inputs, one per branch and side, and
the reference's answers to damaged streams (README.edge.md beside it; oracle/make_rans_edge.py made it with
oracle/_ref/rans_ref) - with what the rANS edge tests share with that script: the damage draw, the call of the driver,
and DEVIATIONS, the list of streams on which this project deliberately does not follow the reference.

  load()                    the fixture: .cases, .bases, .damaged
  run_driver(records, ..)   the reference's answers to [(op, arg, paint, dirty, bytes)]
  answers_ab(calls)         ... twice, as runs A and B of the stability recipe: the answer, None where it is not stable
  damage(rng, stream, ..)   one damaged copy of a stream, as a list of edits
  deviation(codec, stream)  the DEVIATIONS entries whose predicates the stream's bytes satisfy

Test infrastructure only: nothing in htscodecs_amd/ imports this module."""
import collections
import functools
import hashlib
import json
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = os.path.join(ROOT, "tests", "golden", "rans", "edge.bin")
README = os.path.join(ROOT, "tests", "golden", "rans", "README.edge.md")
DRIVER = os.path.join(ROOT, "oracle", "_ref", "rans_ref")
MAGIC = b"RANSEDG1\n"

OP_C16, OP_U16_TO, OP_U16, OP_C8, OP_U8 = range(5)
REFUSED, MADE, REPORT = range(3)
X_PACK, X_RLE, X_CAT, X_NOSZ, X_STRIPE, X_ORDER = 0x80, 0x40, 0x20, 0x10, 0x08, 0x01

# A case: one input and the reference's stream for it under each of `vectors`' orders.  spec: "" where `data` holds the
# input's bytes, else the JSON of a tests/datagen.py spec, and data = (length, sha256).  A vector's stream: bytes, or
# (length, sha256) for the large ones.
Case = collections.namedtuple("Case", "name codec spec data vectors")
Vector = collections.namedtuple("Vector", "order stream")
# A damaged stream: `edits` applied to bases[base]; op/capacity say how it was handed to the reference (OP_U16_TO with a
# capacity, OP_U16, OP_U8); answer: None (unstable), REFUSED, or (length, sha256).
Damaged = collections.namedtuple("Damaged", "base op capacity edits answer")
Fixture = collections.namedtuple("Fixture", "cases bases damaged")


def digest(b):
    return (len(b), hashlib.sha256(bytes(b)).digest())


def case_input(c):
    if not c.spec:
        return c.data
    import datagen
    data = datagen.make(json.loads(c.spec)).tobytes()
    assert digest(data) == c.data, c.name
    return data


def apply(stream, edits):
    """edits: ("cut", length) | ("put", offset, bytes) - inside the stream as it then is."""
    b = bytearray(stream)
    for e in edits:
        if e[0] == "cut":
            assert e[1] <= len(b)
            del b[e[1]:]
        else:
            assert e[1] + len(e[2]) <= len(b)
            b[e[1]:e[1] + len(e[2])] = e[2]
    return bytes(b)


# ---- the fixture's layout --------------------------------------------------------------------------------------------
def _blob(v):
    if isinstance(v, tuple):
        return b"\x01" + v[0].to_bytes(4, "little") + v[1]
    return b"\x00" + len(v).to_bytes(4, "little") + bytes(v)


def write(path, fx):
    out = bytearray(MAGIC + len(fx.cases).to_bytes(4, "little"))
    for c in fx.cases:
        name, spec = c.name.encode(), c.spec.encode()
        out += len(name).to_bytes(2, "little") + name + bytes([c.codec]) + len(spec).to_bytes(2, "little") + spec
        out += _blob(c.data) + len(c.vectors).to_bytes(2, "little")
        for v in c.vectors:
            out += v.order.to_bytes(4, "little") + _blob(v.stream)
    out += len(fx.bases).to_bytes(4, "little")
    for codec, stream in fx.bases:
        out += bytes([codec]) + _blob(stream)
    out += len(fx.damaged).to_bytes(4, "little")
    for d in fx.damaged:
        out += d.base.to_bytes(2, "little") + bytes([d.op]) + d.capacity.to_bytes(4, "little") + bytes([len(d.edits)])
        for e in d.edits:
            if e[0] == "cut":
                out += b"\x01" + e[1].to_bytes(4, "little")
            else:
                out += b"\x00" + e[1].to_bytes(4, "little") + len(e[2]).to_bytes(2, "little") + e[2]
        if d.answer is None:
            out += b"\x00"
        elif d.answer == REFUSED:
            out += b"\x01"
        else:
            out += b"\x02" + d.answer[0].to_bytes(4, "little") + d.answer[1]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(out)


@functools.lru_cache(maxsize=None)
def load():
    with open(EDGE, "rb") as f:
        buf = f.read()
    assert buf[:len(MAGIC)] == MAGIC
    at = len(MAGIC)

    def u(n):
        nonlocal at
        at += n
        assert at <= len(buf)
        return int.from_bytes(buf[at - n:at], "little")

    def take(n):
        nonlocal at
        at += n
        assert at <= len(buf)
        return bytes(buf[at - n:at])

    def blob():
        if u(1):
            return (u(4), take(32))
        return take(u(4))

    cases = []
    for _ in range(u(4)):
        name = take(u(2)).decode()
        codec = u(1)
        spec = take(u(2)).decode()
        data = blob()
        cases.append(Case(name, codec, spec, data, tuple(Vector(u(4), blob()) for _ in range(u(2)))))
    bases = tuple((u(1), blob()) for _ in range(u(4)))
    damaged = []
    for _ in range(u(4)):
        base, op, capacity = u(2), u(1), u(4)
        edits = []
        for _ in range(u(1)):
            if u(1):
                edits.append(("cut", u(4)))
            else:
                off = u(4)
                edits.append(("put", off, take(u(2))))
        kind = u(1)
        damaged.append(Damaged(base, op, capacity, tuple(edits), None if kind == 0 else REFUSED if kind == 1 else (u(4), take(32))))
    assert at == len(buf)
    return Fixture(tuple(cases), bases, tuple(damaged))


def damaged_streams(codec):
    """[(Damaged, stream bytes)] of one codec (16 / 8), in the fixture's order."""
    fx = load()
    return [(d, apply(fx.bases[d.base][1], d.edits)) for d in fx.damaged if fx.bases[d.base][0] == codec]


# ---- the driver ------------------------------------------------------------------------------------------------------
def run_driver(records, env=None, nproc=8):
    """[(answer, value, bytes)] of oracle/_ref/rans_ref over records = [(op, arg, paint, dirty, bytes)]: nproc runs of the
    host program side by side, each over a slice.  env: additions to the environment the program starts in."""
    full = dict(os.environ)
    for k in ("MALLOC_PERTURB_", "ASAN_OPTIONS", "UBSAN_OPTIONS"):
        full.pop(k, None)
    full.update(env or {})
    out = [None] * len(records)
    with tempfile.TemporaryDirectory() as tmp:
        runs = []
        for p in range(min(nproc, max(1, len(records)))):
            part = records[p::nproc]
            src, dst = os.path.join(tmp, "in%d" % p), os.path.join(tmp, "out%d" % p)
            with open(src, "wb") as f:
                f.write(len(part).to_bytes(4, "little"))
                for op, arg, paint, dirty, data in part:
                    f.write(b"".join(v.to_bytes(4, "little") for v in (op, arg, paint, dirty, len(data))) + bytes(data))
            runs.append((p, part, dst, subprocess.Popen([DRIVER, src, dst], env=full, stdout=subprocess.PIPE, stderr=subprocess.PIPE)))
        for p, part, dst, proc in runs:
            _, err = proc.communicate(timeout=1800)
            assert proc.returncode == 0, (proc.returncode, err[-2000:])
            with open(dst, "rb") as f:
                buf = f.read()
            u = lambda at: int.from_bytes(buf[at:at + 4], "little")
            assert u(0) == len(part)
            at = 4
            for k in range(len(part)):
                answer, value = u(at), u(at + 4)
                n = value if answer == MADE else 0
                out[p + k * nproc] = (answer, value, buf[at + 8:at + 8 + n])
                at += 8 + n
            assert at == len(buf)
    return out


# Run A: the stack painted 0x00, the codecs' tables as a first call finds them, every heap block filled with 0x00.
# Run B: the stack painted 0xA5, the tables as an earlier call left them, every heap block filled with 0x5A (90): glibc's
# own fill (MALLOC_PERTURB_) and, for the sanitizer's allocator, which stands in for glibc's in the driver, its own
# (malloc_fill_byte, without its default limit of 4 KiB a block).  Neither is a preload.
RUN_A = (0x00, 0, {"ASAN_OPTIONS": "malloc_fill_byte=0:max_malloc_fill_size=268435456"})
RUN_B = (0xA5, 1, {"MALLOC_PERTURB_": "90", "ASAN_OPTIONS": "malloc_fill_byte=90:max_malloc_fill_size=268435456"})


def answers_ab(calls):
    """calls = [(op, arg, bytes)] -> [answer]: REFUSED or the bytes where runs A and B agree, None where they differ or
    either ended in a report."""
    a, b = (run_driver([(op, arg, paint, dirty, data) for op, arg, data in calls], env) for paint, dirty, env in (RUN_A, RUN_B))
    out = []
    for ra, rb in zip(a, b):
        if ra != rb or ra[0] == REPORT:
            out.append(None)
        else:
            out.append(REFUSED if ra[0] == REFUSED else ra[2])
    return out


# ---- damage ----------------------------------------------------------------------------------------------------------
def damage(rng, stream, codec):
    """One damaged copy of a reference-made stream, as edits for apply(): bit flips, a truncation, the flag byte, the size
    field or table bytes overwritten, a short splice from elsewhere in the stream.  A size field (4x16: the first; 4x8: the
    uncompressed size) stays below 1 MiB; a stripe stream keeps an N above 0."""
    n = len(stream)
    kind = rng.choice(("flip", "flip", "flips", "cut", "flag", "size", "table", "table", "splice"))
    head = 9 if codec == 8 else 1
    if kind == "flip":
        at = rng.randrange(n)
        edits = [("put", at, bytes([stream[at] ^ 1 << rng.randrange(8)]))]
    elif kind == "flips":
        edits = []
        for _ in range(rng.randrange(2, 5)):
            at = rng.randrange(n)
            edits.append(("put", at, bytes([stream[at] ^ 1 << rng.randrange(8)])))
    elif kind == "cut":
        keep = rng.randrange(1, n)
        edits = [("cut", keep)]
        if codec == 8 and keep >= 9 and rng.random() < 0.7:
            edits.append(("put", 1, (keep - 9).to_bytes(4, "little")))
    elif kind == "flag":
        if codec == 8:
            edits = [("put", 0, bytes([rng.choice((0, 1, 1, 2, 255))]))]
        else:
            edits = [("put", 0, bytes([stream[0] ^ rng.choice((1, 0x20, 0x40, 0x80, 0x41, 0xc0, 0x21)) if rng.random() < 0.8 else rng.randrange(256)]))]
    elif kind == "size":
        if codec == 8:
            field = rng.choice((1, 5))
            old = int.from_bytes(stream[field:field + 4], "little")
            new = max(0, old + rng.choice((-9, -1, 1, 2, 64))) if rng.random() < 0.8 else rng.randrange(1 << 20)
            edits = [("put", field, new.to_bytes(4, "little"))]
        else:
            edits = [("put", 1, bytes([rng.randrange(128)]))] if n > 1 else []
    elif kind == "table":
        at = rng.randrange(head, min(n, head + 48))
        edits = [("put", at, bytes([rng.choice((0, 1, stream[at] ^ 0x80, (stream[at] + 1) & 255, (stream[at] - 1) & 255, rng.randrange(256)))]))]
    else:
        size = rng.randrange(1, min(9, n))
        src, dst = rng.randrange(n - size + 1), rng.randrange(n - size + 1)
        edits = [("put", dst, bytes(stream[src:src + size]))]
    out = apply(stream, edits)
    if codec == 16 and len(out) > 0 and out[0] & X_STRIPE:
        _, used = varint(out, 1)
        if 1 + used < len(out) and out[1 + used] == 0:
            edits.append(("put", 1 + used, b"\x04"))
    if codec == 16 and size_field(apply(stream, edits)) >= 1 << 20:
        edits.append(("put", 1, b"\x05"))
    if codec == 8 and len(out) >= 9 and int.from_bytes(out[5:9], "little") >= 1 << 20:
        edits.append(("put", 7, b"\0\0"))
    return edits


# ---- reading a stream's head -----------------------------------------------------------------------------------------
def varint(b, at):
    """(value, bytes used) of the 7-bit big-endian varint at b[at:] (var_get_u32: at most 5 bytes, ends with the input)."""
    v, used = 0, 0
    while at + used < len(b) and used < 5:
        c = b[at + used]
        used += 1
        v = ((v << 7) | (c & 0x7f)) & 0xffffffff
        if not c & 0x80:
            break
    return v, used


def size_field(b):
    """The uncompressed size a 4x16 stream states (0 for X_NOSZ without X_STRIPE, or for an empty stream)."""
    if len(b) < 2 or (b[0] & X_NOSZ and not b[0] & X_STRIPE):
        return 0
    return varint(b, 1)[0]


# ---- random inputs and flag sets (the base streams of the damage draw; the live differential) ----------------------------
def random_input(rng, max_n):
    """0 .. max_n bytes of one of six kinds: uniform over an alphabet, runs, a chain, skewed, text-like, one symbol."""
    n = rng.choice((rng.randrange(0, 40), rng.randrange(0, max_n + 1), rng.randrange(0, max_n + 1)))
    kind = rng.randrange(6)
    nsym = rng.choice((1, 2, 3, 4, 5, 16, 17, 40, 256))
    lo = rng.randrange(0, 257 - nsym)
    if kind == 0:
        return bytes(lo + rng.randrange(nsym) for _ in range(n))
    if kind == 1:
        out = bytearray()
        while len(out) < n:
            out += bytes([lo + rng.randrange(nsym)]) * rng.choice((1, 2, 3, 7, 30, 300))
        return bytes(out[:n])
    if kind == 2:
        out, cur = bytearray(), 0
        for _ in range(n):
            cur = rng.randrange(nsym) if rng.random() < 0.3 else (cur + rng.randrange(-1, 2)) % nsym
            out.append(lo + cur)
        return bytes(out)
    if kind == 3:
        return bytes(lo + min(nsym - 1, int(rng.expovariate(1.0))) for _ in range(n))
    if kind == 4:
        word = bytes(lo + rng.randrange(nsym) for _ in range(rng.randrange(1, 20)))
        return (word * (n // len(word) + 1))[:n]
    return bytes([lo]) * n


def random_order(rng, stripe=True):
    """A 4x16 order argument: any flag set with bits 1 and 2 clear; under X_STRIPE an N of 2 .. 8 in bits 8 and up."""
    order = rng.choice((0, 1)) | rng.choice((0, 0, X_PACK)) | rng.choice((0, 0, X_RLE)) | rng.choice((0, 0, 0, X_CAT)) | rng.choice((0, 0, 0, X_NOSZ))
    if stripe and rng.random() < 0.2:
        order |= X_STRIPE | rng.randrange(2, 9) << 8
    return order


# ---- the streams on which this project does not follow the reference (oracle/rans4x8_oracle.c) ----------------
# Statuses of include/rans4x16_hip.h.
TABLE, SIZE, UNSUPPORTED, CONTEXT = 3, 5, 6, 7


def leaves16(b, capacity=0, plane=None, depth=0):
    """The entropy-coded payloads of a 4x16 stream, found from its bytes as rans_uncompress_to_4x16 finds them (:1352-1595):
    [dict(plane, flags, src, at, order, nested_stripe)] - src[at] is where the order-0 / order-1 payload starts, `at` None
    where the stream ends before it or holds none (X_CAT, nothing left); src is the stream, or what a plane is handed.  A plane that is itself a stripe stream is reported, not
    entered."""
    if not b:
        return []
    flags = b[0]
    if flags & X_STRIPE:
        if depth:
            return [dict(plane=plane, flags=flags, at=None, order=0, nested_stripe=True, src=b)]
        ulen, used = varint(b, 1)
        at = 1 + used
        if at >= len(b):
            return []
        n = b[at]
        at += 1
        clen = []
        for _ in range(n):
            v, used = varint(b, at)
            at += used
            clen.append(v)
            if at > len(b) or v > len(b) or v < 1:
                return []
        if at + sum(clen) > len(b):
            return []
        out = []
        for i, v in enumerate(clen):
            out += leaves16(b[at:at + sum(clen[i:])], ulen // n + (ulen % n > i), i, 1)
            at += v
        return out
    at = 1
    if not flags & X_NOSZ:
        at += varint(b, 1)[1]
    leaf = dict(plane=plane, flags=flags, at=None, order=flags & 1, nested_stripe=False, src=b)
    if flags & X_PACK:
        if at >= len(b):
            return [leaf]
        n = b[at] or 256                                          # hts_unpack_meta, pack.c:165-198
        if n > 16:
            at += 1
        elif len(b) - at <= 1:
            return [leaf]
        else:
            at += 1 + min(n, len(b) - at - 1)
        at += varint(b, at)[1]
    if flags & X_RLE:
        meta, used = varint(b, at)
        at += used
        at += varint(b, at)[1]
        if meta & 1:
            at += min(meta // 2, max(0, len(b) - at))
        else:
            csz, used = varint(b, at)
            at += used + csz
    if at < len(b) and not flags & X_CAT:
        leaf["at"] = at
    return [leaf]


def o1_table(b, at):
    """(shift, compressed, usz, rows, spans) of the order-1 payload at b[at:]: rows = {context: sum of its row} read from
    an uncompressed table as the reference reads it (:327-358, :959-998), None for a compressed one or one that ends
    early; spans = {context: (first byte of its row, the byte behind it)}."""
    head = b[at]
    shift, compressed = head >> 4, head & 1
    if compressed:
        return shift, 1, varint(b, at + 1)[0], None, None
    end = len(b)
    cp = at + 1
    alpha, run = [], 0
    if cp >= end:
        return shift, 0, 0, None, None
    j = b[cp]
    cp += 1
    more = cp + 2 < end or j
    while more:
        alpha.append(j)
        if cp >= end:
            return shift, 0, 0, None, None
        if not run and j + 1 == b[cp]:
            if cp + 1 >= end:
                return shift, 0, 0, None, None
            j, run = b[cp], b[cp + 1]
            cp += 2
        elif run:
            run -= 1
            j += 1
            if j > 255:
                return shift, 0, 0, None, None
        else:
            j = b[cp]
            cp += 1
        more = j and cp < end
    alpha = sorted(set(alpha))
    rows, spans = {}, {}
    for c in alpha:
        tot, zeros, first = 0, 0, cp
        if cp >= end:
            return shift, 0, 0, None, None
        for _ in alpha:
            if cp >= end:
                break
            if zeros:
                zeros -= 1
                continue
            f, used = varint(b, cp)
            cp += used
            if f == 0:
                if cp >= end:
                    return shift, 0, 0, None, None
                zeros = b[cp]
                cp += 1
            tot += f
        rows[c] = tot
        spans[c] = (first, cp)
    return shift, 0, 0, rows, spans


def _o1_leaves(b, capacity):
    return [(leaf, o1_table(leaf["src"], leaf["at"])) for leaf in leaves16(bytes(b), capacity) if leaf["at"] is not None and leaf["order"]]


def tables8(b):
    """What the tables of a 4x8 stream say, read as the reference reads them (rANS_static.c:274-310, :748-813), or None where
    the read fails: dict(order, ascending, listed (every byte listed as a context or a symbol), rows = [(context, row number,
    total)] in listing order, end = where the four states start).  The reference numbers the rows of an order-1 stream by first appearance, context or symbol."""
    n = len(b)
    if n < 26 or b[0] > 1 or (b[0] and n < 27):
        return None
    g = lambda k: b[k] if k < n else 0
    number, rows, ascending = {}, [], True

    def table(cp, zero_is_total):
        x = rle = 0
        j = g(cp)
        cp += 1
        prev = -1
        nonlocal ascending
        while True:
            number.setdefault(j, len(number))
            if cp > n - 16:
                return None
            f = g(cp)
            cp += 1
            if f >= 128:
                f = (f & 127) << 8 | g(cp)
                cp += 1
            if not f and zero_is_total:
                f = 4096
            if x + f > 4096:
                return None
            ascending &= j > prev
            prev = j
            x += f
            if not rle and j + 1 == g(cp):
                j, rle = g(cp), g(cp + 1)
                cp += 2
            elif rle:
                rle -= 1
                j += 1
                if j > 255:
                    return None
            else:
                j = g(cp)
                cp += 1
            if not j:
                break
        return (cp, x) if 4095 <= x <= 4096 else None

    if b[0] == 0:
        r = table(9, False)
        if r is None:
            return None
        return dict(order=0, ascending=ascending, listed=set(number), rows=[(0, 0, r[1])], end=r[0])
    cp, rle_i, prev = 9, 0, -1
    i = g(cp)
    cp += 1
    while True:
        number.setdefault(i, len(number))
        was = ascending
        r = table(cp, True)
        if r is None:
            return None
        ascending = was and ascending and i > prev
        prev = i
        cp = r[0]
        rows.append((i, number[i], r[1]))
        if not rle_i and i + 1 == g(cp):
            i, rle_i = g(cp), g(cp + 1)
            cp += 2
        elif rle_i:
            rle_i -= 1
            i += 1
            if i > 255:
                return None
        else:
            i = g(cp)
            cp += 1
        if not i:
            break
    return dict(order=1, ascending=ascending, listed=set(number), rows=rows, end=cp)


def _shift_below_10(b, capacity):
    return any(t[0] < 10 for _, t in _o1_leaves(b, capacity))


def _row_missing_behind_first_plane(b, capacity):
    """A plane behind the first whose raw order-1 table has a context without a row: one whose frequencies are all zero
    (:977 skips it), or context 0, in which every quarter starts, outside the alphabet."""
    return any(leaf["plane"] and t[3] and (0 in t[3].values() or 0 not in t[3]) for leaf, t in _o1_leaves(b, capacity))


def _nested_table_large(b, capacity):
    return any(t[1] and t[2] > 204800 for _, t in _o1_leaves(b, capacity))


def _nested_stripe(b, capacity):
    return any(leaf["nested_stripe"] for leaf in leaves16(bytes(b), capacity))


def _x8_not_ascending(b, capacity):
    t = tables8(b)
    return t is not None and not t["ascending"]


def _x8_slot_4095_first_step(b, capacity):
    """Context 0 is listed first (the reference numbers rows by first appearance, :751-759, so its row is row 0 and the
    copy of slot 4094 to slot 4095 of row <context byte>, :799-800, lands in its own row), its table sums to 4095, and
    one of the four initial states that decode a byte points at slot 4095: the first look-up of that quarter, in context
    0, is of the slot that oracle and device refuse and the reference has filled from this call's bytes."""
    t = tables8(b)
    if t is None or not t["order"] or t["rows"][0] != (0, 0, 4095) or t["end"] + 16 > len(b):
        return False
    out_sz = int.from_bytes(b[5:9], "little")
    decodes = [out_sz >= 4, out_sz >= 4, out_sz >= 4, out_sz >= 1]
    return any(d and int.from_bytes(b[t["end"] + 4 * k:t["end"] + 4 * k + 2], "little") & 4095 == 4095 for k, d in enumerate(decodes))


def _x8_byte_0_unlisted(b, capacity):
    t = tables8(b)
    return t is not None and t["order"] == 1 and 0 not in t["listed"]


def _x8_encode_nothing(b, capacity):
    return len(b) == 0


# oracle: what the oracle does on a member whose reference answer is stable and accepted - "refuses", "other" (accepts,
# with other bytes) or "follows" (the reference's answer: the deviation is the device's alone).  status: the device's.
Deviation = collections.namedtuple("Deviation", "name codec what predicate status oracle why")
DEVIATIONS = (
    Deviation("o1_shift_below_10", 16, "decode", _shift_below_10, UNSUPPORTED, "refuses",
              "an order-1 payload whose header states a shift below 10: the reference looks up 10 bits in rows it filled to 2^shift"),
    Deviation("o1_row_missing_behind_first_plane", 16, "decode", _row_missing_behind_first_plane, CONTEXT, "other",
              "an order-1 plane behind the first of a stripe stream with a context that has no row: the reference decodes it "
              "from what the plane before left in its tables; the oracle restates such a row as zeros, the device refuses its use"),
    Deviation("nested_table_above_204800", 16, "decode", _nested_table_large, UNSUPPORTED, "follows",
              "an order-1 table sent as an order-0 stream of more than 204,800 bytes: no valid table is that large"),
    Deviation("nested_stripe", 16, "decode", _nested_stripe, UNSUPPORTED, "follows",
              "a plane of a stripe stream that is itself a stripe stream"),
    Deviation("x8_not_ascending", 8, "decode", _x8_not_ascending, TABLE, "follows",
              "a 4x8 table that lists symbols or contexts out of ascending order: the reference assigns slots in listing order"),
    Deviation("x8_slot_4095_first_step", 8, "decode", _x8_slot_4095_first_step, TABLE, "refuses",
              "slot 4095 of context 0's 4095-sum table, looked up by a quarter's initial state: the reference's copy of slot 4094 is there"),
    Deviation("x8_byte_0_unlisted", 8, "decode", _x8_byte_0_unlisted, CONTEXT, "refuses",
              "a 4x8 order-1 stream that lists byte 0 nowhere: the quarters start in context 0, which the reference sends to its first row"),
    Deviation("x8_encode_nothing", 8, "encode", _x8_encode_nothing, SIZE, "refuses",
              "rans_compress of 0 bytes: the reference divides by zero"),
)


def deviation(codec, stream, capacity=0, what="decode"):
    """The DEVIATIONS entries whose predicate the bytes satisfy."""
    return [d for d in DEVIATIONS if d.codec == codec and d.what == what and d.predicate(bytes(stream), capacity)]
