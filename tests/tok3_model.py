"""Python model of the tok3 column container (htscodecs tokenise_name3.c:1431-1531 and :1546-1669), for the tok3 tests.

Two verdicts per container:
  walk(buf, ..)           ours - include/rans4x16_hip.h part 2c, the stricter cases included - with the status code
  reference_accepts(buf)  the reference's own walk rules (pass / fail), the rANS streams left to the oracle
and the framing of encode_names over streams the oracle compressed (frame()).

Test infrastructure only: nothing in htscodecs_amd/ imports this module."""
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tok3")

OK, CAPACITY, TRUNCATED, SIZE, UNSUPPORTED, EMPTY = 0, 1, 2, 5, 6, 9
N_MATCH = 10
MAX_TOKENS = 128
PLAIN, DUP, SYNTH = "plain", "dup", "synth"

# the method lists of the fixtures' levels (the build that made them; ISSUE / DESIGN 4.5), and the fixtures that do not
# re-frame byte for byte from their own columns (made without the in_len % 4 skip of :1270)
LISTS = {1: [0], 3: [0, 200], 5: [0, 201], 7: [0, 1, 129, 65, 193, 201], 9: [0, 1, 128, 129, 64, 65, 192, 193, 201]}
EXCEPTIONS = ("20.names.3", "rr.names.3", "20.names.5", "rr.names.5")
# the method lists of the reference at the version this project was modelled on (tokenise_name3.c:1255-1261, both
# flavours): what made tests/golden/tok3/edge.bin and the arith fixtures, and what the level of the host calls stands for
REF_LISTS = {1: [0, 128], 3: [0, 200], 5: [0, 128, 201], 7: [0, 1, 129, 65, 193, 201], 9: [0, 1, 128, 129, 64, 65, 192, 193, 201]}


def fixtures():
    """[(name, bytes)] of the 55 rANS containers, sorted by name."""
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "*.names.[13579]"))):
        with open(p, "rb") as f:
            out.append((os.path.basename(p), f.read()))
    return out


def level_of(name):
    return int(name.rsplit(".", 1)[1])


def var_put(v):
    groups = [v & 0x7F]
    v >>= 7
    while v:
        groups.append(v & 0x7F)
        v >>= 7
    return bytes([g | (0x80 if i else 0) for i, g in reversed(list(enumerate(groups)))])


def var_get(buf, pos, end):
    """varint.h:131-160 over buf[pos:end]: (value, bytes used, last byte still continued); used 0 if there is none."""
    if pos >= end:
        return 0, 0, False
    v, p = 0, pos
    while True:
        c = buf[p]
        p += 1
        v = ((v << 7) | (c & 0x7F)) & 0xFFFFFFFF
        if not (c & 0x80) or p >= end:
            return v, p - pos, bool(c & 0x80)


class Walk:
    def __init__(self):
        self.status = OK
        self.last_start = self.nreads = self.ndesc = 0
        self.cols = []       # dicts: id, kind, size, and stream_off / clen (plain), src (dup: column index or None), type (synth)

    @property
    def ncol(self):
        return len(self.cols)

    @property
    def total(self):
        return sum(c["size"] for c in self.cols)

    @property
    def largest_col(self):
        return max([c["size"] for c in self.cols] or [0])

    @property
    def largest_stream(self):
        return max([c["clen"] for c in self.cols if c["kind"] == PLAIN] or [0])


def walk(buf, max_columns=2048, max_col_size=0xFFFFFFFF):
    """Our walk.  Returns a Walk; after a failure .cols holds the columns accepted before it."""
    w = Walk()

    done = [0, 0]                              # columns and descriptors accepted so far

    def fail(st):
        w.status = st
        del w.cols[done[0]:]                   # (a type column goes with the descriptor that opened its position)
        w.ndesc = done[1]
        return w

    size = len(buf)
    if size < 9:
        return fail(TRUNCATED)
    w.last_start = int.from_bytes(buf[0:4], "little")
    w.nreads = int.from_bytes(buf[4:8], "little")
    if buf[8] != 0:
        return fail(UNSUPPORTED)
    if w.last_start >= 0x7FFFFFFF - 1024:
        return fail(SIZE)
    o, tnum, last_id = 9, -1, -1
    by_id = {}
    while o < size:
        if w.ndesc >= max_columns:
            return fail(UNSUPPORTED)
        t = buf[o]
        o += 1
        w.ndesc += 1
        j = None
        if t & 64:
            if o + 2 >= size:
                return fail(TRUNCATED)
            j = (buf[o] << 4) + buf[o + 1]
            o += 2
        if t & 128:
            tnum += 1
            if tnum >= MAX_TOKENS:
                return fail(SIZE)
            if t & 15:
                if w.nreads == 0:
                    return fail(SIZE)
                if w.nreads > max_col_size:
                    return fail(UNSUPPORTED)
                by_id[tnum << 4] = w.ncol
                w.cols.append({"id": tnum << 4, "kind": SYNTH, "type": t & 15, "size": w.nreads})
                last_id = tnum << 4
        if tnum < 0:
            return fail(SIZE)
        cid = (tnum << 4) | (t & 15)
        if j is not None and j >= cid:
            return fail(SIZE)
        if cid <= last_id:
            return fail(UNSUPPORTED)
        if j is not None:
            src = by_id.get(j)
            if src is None or w.cols[src]["size"] == 0:
                col = {"id": cid, "kind": DUP, "src": None, "size": 0}
            else:
                col = {"id": cid, "kind": DUP, "src": src, "size": w.cols[src]["size"]}
        else:
            clen, nb, cont = var_get(buf, o, size)
            if nb == 0 or cont:
                return fail(TRUNCATED)
            so = o + nb
            if clen > size - so:
                return fail(TRUNCATED)
            if clen == 0:
                return fail(EMPTY)
            flags = buf[so]
            if (flags & 0x10) and not (flags & 0x08):
                return fail(SIZE)
            claim, ub, cont = var_get(buf, so + 1, so + clen)
            if ub == 0 or cont:
                return fail(TRUNCATED)
            if claim > max_col_size:
                return fail(UNSUPPORTED)
            col = {"id": cid, "kind": PLAIN, "stream_off": so, "clen": clen, "size": claim}
            o = so + clen
        by_id[cid] = w.ncol
        w.cols.append(col)
        last_id = cid
        done[:] = [len(w.cols), w.ndesc]
    if w.total > 0xFFFFFFFF:
        return fail(UNSUPPORTED)
    return w


def reference_accepts(buf, decode):
    """The reference's decode_names up to the per-name decoder (:1546-1669): True / False.  decode(stream bytes, ulen) ->
    bytes or None is the codec (the oracle); the stream handed to it is the rest of the container, as the reference does."""
    sz = len(buf)
    if sz < 9:
        return False
    ulen = int.from_bytes(buf[0:4], "little")
    if ulen >= 0x7FFFFFFF - 1024:
        return False
    nreads = int.from_bytes(buf[4:8], "little")
    if nreads >= 0x80000000:
        return False                          # (create_context refuses / cannot allocate)
    if buf[8] != 0:
        return False                          # the arithmetic coder: out of scope
    o, tnum = 9, -1
    while o < sz:
        t = buf[o]
        o += 1
        if t & 64:
            if o + 2 >= sz:
                return False
            j = (buf[o] << 4) + buf[o + 1]
            o += 2
            if t & 128:
                tnum += 1
                if tnum >= MAX_TOKENS:
                    return False
            if (t & 15) and (t & 128) and nreads == 0:
                return False                  # (writes buf[0] of a zero-byte allocation: we refuse)
            if tnum < 0:
                return False
            if j >= ((tnum << 4) | (t & 15)):
                return False
            continue
        if t & 128:
            tnum += 1
            if tnum >= MAX_TOKENS:
                return False
        if (t & 15) and (t & 128) and nreads == 0:
            return False
        if o >= sz:
            return False                      # (reads past the end: we refuse)
        clen, nb, _ = var_get(buf, o, sz)
        claim, _, _ = var_get(buf, o + nb + 1, sz)
        if tnum < 0:
            return False
        if decode(bytes(buf[o + nb:]), claim) is None:
            return False
        o += clen + nb
    return True


def columns(buf, w, decode):
    """The bytes of every column of a walked container (w.status == OK): decode(stream, size) for the plain ones.
    Returns a list of bytes, or None where the codec refuses a stream."""
    out = []
    for c in w.cols:
        if c["kind"] == PLAIN:
            d = decode(bytes(buf[c["stream_off"]:c["stream_off"] + c["clen"]]), c["size"])
            if d is None or len(d) != c["size"]:
                return None
            out.append(d)
        elif c["kind"] == SYNTH:
            out.append(bytes([c["type"]]) + bytes([N_MATCH]) * (c["size"] - 1))
        else:
            out.append(out[c["src"]] if c["src"] is not None else b"")
    return out


def described(w):
    """The columns of a walk that have a descriptor of their own - what encode_names was given: [(id, index)]."""
    return [(c["id"], i) for i, c in enumerate(w.cols) if c["kind"] != SYNTH]


def best(compress, data, methods):
    """compress() of tokenise_name3.c:1246-1300: (method, stream) of the smallest result, the first winning ties."""
    win = None
    for m in methods:
        if len(data) % 4 != 0 and (m & 8):
            continue
        s = compress(data, m)
        assert s is not None
        if win is None or len(s) < len(win[1]):
            win = (m, s)
    return win


def frame(compress, cols, methods, last_start, nreads):
    """encode_names :1431-1531 over cols = [(id, bytes)] with ascending ids.  Returns (container, [method per column])."""
    out = bytearray(last_start.to_bytes(4, "little") + nreads.to_bytes(4, "little") + b"\0")
    seen = []                                  # (id, varint + stream)
    chosen = []
    last_tnum = -1
    for cid, data in cols:
        m, s = best(compress, data, methods)
        chosen.append(m)
        full = var_put(len(s)) + s
        dup_from = 0
        for jid, other in seen:
            if len(other) == len(full) and len(full) > 4 and other == full:
                dup_from = jid
                break
        seen.append((cid, full))
        t = cid & 15
        if cid >> 4 != last_tnum:
            t |= 128
            last_tnum = cid >> 4
        if dup_from:
            out += bytes([t | 64, dup_from >> 4, dup_from & 15])
        else:
            out += bytes([t]) + full
    return bytes(out), chosen
