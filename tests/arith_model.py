"""A Python restatement of htscodecs' adaptive arithmetic codec (arith_dynamic.c with c_simple_model.h and
c_range_coder.h): the range coder, the adaptive model with its list order kept exactly, the four core decoders and
encoders, arith_compress_to and arith_uncompress_to.  It is the checker of the arith tests and is itself pinned by the
reference-made files of tests/golden/arith (test_arith_cpu.py), by nothing made from itself.

uncompress_to gives (status, bytes): the statuses are those of htscodecs_amd/csrc/r4x16_arith_parse.h, status 0 where the
reference returns a buffer, another code where it returns NULL."""
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "arith")

X_PACK, X_RLE, X_CAT, X_NOSZ, X_STRIPE, X_EXT = 0x80, 0x40, 0x20, 0x10, 0x08, 0x04
OK, E_CAPACITY, E_TRUNCATED, E_SIZE, E_UNSUPPORTED, E_EMPTY = 0, 1, 2, 5, 6, 9     # R4X16_E_* of include/rans4x16_hip.h
MAX_FREQ = (1 << 16) - 17
STEP = 16
TOP = 1 << 24
M32 = 0xffffffff
INT_MAX = 0x7fffffff


# ---- varint.h (big endian, 7 bits a byte) ------------------------------------------------------------------------
def var_put(v):
    out = [v & 0x7f]
    v >>= 7
    while v:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    return bytes(reversed(out))


def var_get(buf, pos, end):
    """(bytes consumed, value): varint.h:131-160 over [pos, end)"""
    if pos >= end:
        return 0, 0
    v, p = 0, pos
    while True:
        c = buf[p]
        p += 1
        v = ((v << 7) | (c & 0x7f)) & M32
        if not (c & 0x80) or p >= end:
            return p - pos, v


# ---- c_simple_model.h --------------------------------------------------------------------------------------------
class Model:
    """F / S: frequency and symbol of each list position, live entries only (the entries behind them have frequency 0
    and are never reached: the normalise loop stops at the first of them, a scan that passes them is an error)."""
    __slots__ = ("F", "S", "tot")

    def __init__(self, max_sym):
        self.F = [1] * max_sym
        self.S = list(range(max_sym))
        self.tot = max_sym

    def _update(self, i):
        F, S = self.F, self.S
        F[i] += STEP
        self.tot += STEP
        if self.tot > MAX_FREQ:
            t = 0
            for k in range(len(F)):
                F[k] -= F[k] >> 1
                t += F[k]
            self.tot = t
        if i > 0 and F[i] > F[i - 1]:                      # (position 0 has the sentinel before it: MAX_FREQ)
            F[i], F[i - 1] = F[i - 1], F[i]
            S[i], S[i - 1] = S[i - 1], S[i]


class Decoder:
    def __init__(self, buf, pos, end):
        """RC_SetInput(in + 1, in + in_size) and RC_StartDecode: c_range_coder.h:56-69"""
        self.buf, self.end = buf, end
        self.range, self.code = M32, 0
        if pos + 5 >= end:
            self.pos = end
        else:
            self.code = int.from_bytes(buf[pos:pos + 5], "big") & M32
            self.pos = pos + 5

    def symbol(self, m):
        tot = m.tot
        if tot and self.range >= tot:
            self.range //= tot
            freq = self.code // self.range
        else:
            freq = 0
        if freq > MAX_FREQ:
            return 0
        F = m.F
        acc, i, n = 0, 0, len(F)
        while i < n:
            acc += F[i]
            if acc > freq:
                break
            i += 1
        else:
            return 0                                        # ran off the list: c_simple_model.h:158
        acc -= F[i]
        self.code = (self.code - acc * self.range) & M32
        self.range = (self.range * F[i]) & M32
        while self.range < TOP:
            if self.pos >= self.end:
                break
            self.code = ((self.code << 8) + self.buf[self.pos]) & M32
            self.pos += 1
            self.range = (self.range << 8) & M32
        sym = m.S[i]
        m._update(i)
        return sym


class Encoder:
    def __init__(self):
        self.low, self.range, self.ffnum, self.carry, self.cache = 0, M32, 0, 0, 0
        self.out = bytearray()

    def _shift_low(self):
        if self.low < 0xff000000 or self.carry:
            self.out.append((self.cache + self.carry) & 0xff)
            while self.ffnum:
                self.out.append((self.carry - 1) & 0xff)
                self.ffnum -= 1
            self.cache = self.low >> 24
            self.carry = 0
        else:
            self.ffnum += 1
        self.low = (self.low << 8) & M32

    def symbol(self, m, sym):
        i = m.S.index(sym)
        acc = sum(m.F[:i])
        tmp = self.low
        self.range //= m.tot
        self.low = (self.low + acc * self.range) & M32
        self.range = (self.range * m.F[i]) & M32
        self.carry += self.low < tmp
        while self.range < TOP:
            self.range = (self.range << 8) & M32
            self._shift_low()
        m._update(i)

    def finish(self):
        for _ in range(5):
            self._shift_low()
        return bytes(self.out)


# ---- the four core coders (arith_dynamic.c:98-614) ---------------------------------------------------------------
def _run_ctx(rctx, last):
    return 256 if rctx == last else rctx + (rctx < 257)


def encode_core(data, order, rle):
    m = (max(data) if data else 0) + 1
    models = [Model(m) for _ in range(256 if order else 1)]
    runs = [Model(4) for _ in range(258)] if rle else None
    rc = Encoder()
    last, i, n = 0, 0, len(data)
    while i < n:
        c = data[i]
        rc.symbol(models[last if order else 0], c)
        last = c
        i += 1
        if not rle:
            continue
        run = 0
        while i < n and data[i] == last:
            run += 1
            i += 1
        rctx = last
        while True:
            part = run if run < 4 else 3
            rc.symbol(runs[rctx], part)
            run -= part
            rctx = _run_ctx(rctx, last)
            if part == 3 and run == 0:
                rc.symbol(runs[rctx], 0)
            if not run:
                break
    return bytes([m & 0xff]) + rc.finish()


def _census_symbol(rc, m, ev, where):
    """Decoder.symbol and Model._update once more, counting what the step did under (where, event): the census of
    decode_core.  `where` is the home of a symbol model ("o0", "o1_lds", "o1_global") or "run" for a run-length model;
    the boundary events - a swap at a list position that is a multiple of 4 above 0 - are a symbol model's alone."""
    tot = m.tot
    if tot and rc.range >= tot:
        rc.range //= tot
        freq = rc.code // rc.range
    else:
        freq = 0
        ev[where, "range_lt_tot"] += 1
    if freq > MAX_FREQ:
        ev[where, "freq_gt_max"] += 1
        return 0
    F, S = m.F, m.S
    acc, i, n = 0, 0, len(F)
    while i < n:
        acc += F[i]
        if acc > freq:
            break
        i += 1
    else:
        ev[where, "ran_off"] += 1
        return 0
    acc -= F[i]
    rc.code = (rc.code - acc * rc.range) & M32
    rc.range = (rc.range * F[i]) & M32
    while rc.range < TOP:
        if rc.pos >= rc.end:
            ev[where, "starved"] += 1
            break
        rc.code = ((rc.code << 8) + rc.buf[rc.pos]) & M32
        rc.pos += 1
        rc.range = (rc.range << 8) & M32
    sym = S[i]
    F[i] += STEP
    m.tot += STEP
    before = i > 0 and F[i] > F[i - 1]
    halved = m.tot > MAX_FREQ
    if halved:
        t = 0
        for k in range(n):
            F[k] -= F[k] >> 1
            t += F[k]
        m.tot = t
    swap = i > 0 and F[i] > F[i - 1]
    if swap:
        F[i], F[i - 1] = F[i - 1], F[i]
        S[i], S[i - 1] = S[i - 1], S[i]
    edge = where != "run" and i > 0 and i % 4 == 0
    for name, on in (("halve", halved), ("swap", swap), ("halve_swap", halved and swap),
                     ("halve_tie", halved and before and not swap)):
        if on:
            ev[where, name] += 1
            if edge and name != "halve":
                ev[where, name + "_boundary"] += 1
    return sym


def _census_core(buf, pos, end, out_sz, order, rle, ev, where):
    """decode_core's loop over _census_symbol, with the events of the run loop (under "run") and the payload's size:
    ev[where, "payload", end - pos] counts the pieces of that size"""
    m = buf[pos] or 256
    models = [Model(m) for _ in range(256 if order else 1)]
    runs = [Model(4) for _ in range(258)] if rle else None
    rc = Decoder(buf, pos + 1, end)
    ev[where, "payload", end - pos] += 1
    if pos + 6 >= end:
        ev[where, "short_start"] += 1
    out = bytearray(out_sz)
    last, i = 0, 0
    while i < out_sz:
        c = _census_symbol(rc, models[last if order else 0], ev, where)
        out[i] = c
        last = c
        if rle:
            run, rctx, trips = 0, last, 0
            while True:
                if rctx == 257:
                    ev["run", "ctx257"] += 1
                r = _census_symbol(rc, runs[rctx], ev, "run")
                rctx = _run_ctx(rctx, last)
                run += r
                trips += 1
                if not (r == 3 and run < out_sz):
                    break
            if trips >= 3:
                ev["run", "chain3"] += 1
            if r == 3:
                ev["run", "chain_cut"] += 1
            if run > out_sz - 1 - i:
                ev["run", "run_clipped"] += 1
            while run and i + 1 < out_sz:
                run -= 1
                i += 1
                out[i] = last
        i += 1
    return bytes(out)


def decode_core(buf, pos, end, out_sz, order, rle, events=None, where=None):
    """arith_uncompress_O0 / O1 / O0_RLE / O1_RLE over buf[pos:end], out_sz bytes; end > pos.  events: a
    collections.Counter that takes the census of this piece (_census_core: the same bytes by a loop that counts), under
    the home `where`; None: nothing is counted."""
    if events is not None:
        return _census_core(buf, pos, end, out_sz, order, rle, events, where)
    m = buf[pos] or 256
    models = [Model(m) for _ in range(256 if order else 1)]
    runs = [Model(4) for _ in range(258)] if rle else None
    rc = Decoder(buf, pos + 1, end)
    out = bytearray(out_sz)
    last, i = 0, 0
    while i < out_sz:
        c = rc.symbol(models[last if order else 0])
        out[i] = c
        last = c
        if rle:
            run, rctx = 0, last
            while True:
                r = rc.symbol(runs[rctx])
                rctx = _run_ctx(rctx, last)
                run += r
                if not (r == 3 and run < out_sz):
                    break
            while run and i + 1 < out_sz:
                run -= 1
                i += 1
                out[i] = last
        i += 1
    return bytes(out)


# ---- pack.c ------------------------------------------------------------------------------------------------------
def hts_pack(data):
    """(meta, packed) - meta of one byte: more than 16 symbols, not packed"""
    syms = sorted(set(data))
    n = len(syms)
    if n > 16:
        return bytes([n & 0xff]), bytes(data)
    meta = bytes([n]) + bytes(syms)
    code = {s: k for k, s in enumerate(syms)}
    per, bits = (2, 4) if n > 4 else (4, 2) if n > 2 else (8, 1) if n > 1 else (0, 0)
    if not per:
        return meta, b""
    out = bytearray((len(data) + per - 1) // per)
    for i, c in enumerate(data):
        out[i // per] |= code[c] << (bits * (i % per))
    return meta, bytes(out)


def _unpack_meta(buf, pos, end):
    """hts_unpack_meta: (bytes consumed or 0, map, nsym)"""
    mp = [0] * 16
    if end <= pos:
        return 0, mp, 0
    n = buf[pos] or 256
    if n > 16:
        return 1, mp, 1
    nsym = 0 if n <= 1 else 8 if n <= 2 else 4 if n <= 4 else 2
    if end - pos <= 1:
        return 0, mp, nsym
    j, c = 1, 0
    while True:
        mp[c] = buf[pos + j]
        c += 1
        j += 1
        if not (c < n and j < end - pos):
            break
    return (0 if c < n else j), mp, nsym


def _unpack(data, out_len, nsym, mp):
    """hts_unpack for nsym 0, 2, 4, 8: None where it refuses"""
    if nsym == 0:
        return bytes([mp[0]]) * out_len
    bits = 8 // nsym
    if (out_len + nsym - 1) // nsym > len(data):
        return None
    mask = (1 << bits) - 1
    return bytes(mp[(data[i // nsym] >> (bits * (i % nsym))) & mask] for i in range(out_len))


# ---- arith_compress_to (arith_dynamic.c:621-863) -------------------------------------------------------------------
STRIPE_METHODS = ((1, 64, 0), (1, 0), (1, 128), (1, 128))


def compress(data, order):
    data = bytes(data)
    n = len(data)
    if n <= 20:
        order &= ~X_STRIPE
    if order & X_STRIPE:
        N = (order >> 8) or 4
        assert N <= 255
        planes = [data[j::N] for j in range(N)]
        head = bytes([order & 0xff & ~X_NOSZ]) + var_put(n) + bytes([N])
        lens, body = b"", b""
        for i, p in enumerate(planes):
            best = None
            for meth in STRIPE_METHODS[min(i, 3)]:
                if (order & 3) == 0 and (meth & 1):
                    continue
                c = compress(p, meth | X_NOSZ)
                if best is None or len(c) < len(best):       # first smallest wins
                    best = c
            lens += var_put(len(best))
            body += best
        return head + lens + body
    flags = order & 0xff
    meta = b"" if flags & X_NOSZ else var_put(n)
    order &= 3
    if flags & X_PACK and n:
        pmeta, packed = hts_pack(data)
        if len(pmeta) == 1 and pmeta[0] > 16:                # (256 symbols: the count wraps to 0 and the flag stays)
            flags &= ~X_PACK
        else:
            data, n = packed, len(packed)
            meta += pmeta + var_put(n)
    elif flags & X_PACK:
        flags &= ~X_PACK
    if flags & X_RLE and not n:
        flags &= ~X_RLE
    if order and n < 8:
        flags &= ~3
        order = 0
    assert not flags & X_EXT, "X_EXT is bzip2: not modelled"
    # (an explicit X_CAT leaves the coders no room, :637-642 and their bound check: the fall-back below stores the bytes)
    body = None if flags & X_CAT else encode_core(data, order == 1, bool(flags & X_RLE))
    if body is None or len(body) >= n:
        flags = (flags & ~(3 | X_EXT)) | X_CAT
        body = data
    return bytes([flags]) + meta + body


# ---- arith_uncompress_to (arith_dynamic.c:870-1114) ----------------------------------------------------------------
def lds_home(m):
    """an order-1 stream's rows in LDS: m rows of m entries padded to four, and m totals, in the 32 KiB a wave has less
    the 258 run-length models (htscodecs_amd/csrc/r4x16_arith.hip)"""
    return m * ((m + 3) // 4 * 4) * 4 + m * 4 <= 32768 - 258 * 16


def _piece(buf, pos, end, cap, trace=None, events=None):
    """One stream without X_STRIPE at buf[pos:end]; cap None: the size comes from the stream.  (status, bytes).
    trace: a list that takes the route kind of the entropy-coded piece, and "rle" if it carries run lengths.
    events: decode_core's census counter."""
    flags = buf[pos]
    p = pos + 1
    if flags & X_NOSZ:
        if cap is None:
            return E_SIZE, b""
        osz = cap
    else:
        nb, osz = var_get(buf, p, end)
        p += nb
    if osz >= INT_MAX:
        return E_SIZE, b""
    if cap is not None and cap < osz:
        return E_CAPACITY, b""
    dec = osz
    nsym, mp = None, None
    if flags & X_PACK:
        nb, mp, nsym = _unpack_meta(buf, p, end)
        if nb == 0:
            return E_TRUNCATED, b""
        p += nb
        nb, dec = var_get(buf, p, end)
        p += nb
        if dec > osz:
            return E_CAPACITY, b""
    if end - p > 0:
        if flags & X_CAT:
            if dec > end - p:
                return E_TRUNCATED, b""
            tmp = bytes(buf[p:p + dec])
        elif flags & X_EXT:
            return E_UNSUPPORTED, b""
        else:
            home = "o0" if (flags & 3) != 1 else "o1_lds" if lds_home(buf[p] or 256) else "o1_global"
            tmp = decode_core(buf, p, end, dec, (flags & 3) == 1, bool(flags & X_RLE), events, home)
            if trace is not None:
                trace.append(home)
                if flags & X_RLE:
                    trace.append("rle")
    else:
        tmp = b""
    if flags & X_PACK:
        if nsym == 1:
            return OK, tmp
        out = _unpack(tmp, osz, nsym, mp)
        return (E_SIZE, b"") if out is None else (OK, out)
    return OK, tmp


def uncompress_to(buf, cap=None, max_planes=255, max_stripe_out=None, trace=None, events=None):
    """arith_uncompress_to(buf, len(buf), out, &cap); cap None: out == NULL.  max_planes / max_stripe_out: what
    rans4x16_hip_set_dev_stripe_planes reserved (the device call's limits; None: no limit).  events: a
    collections.Counter for the census of the pieces of an accepted block (decode_core); a block that is refused counts
    nothing, as in `trace`: the device decodes none of its pieces."""
    if events is None:
        return _uncompress_to(buf, cap, max_planes, max_stripe_out, trace, None)
    mine = type(events)()
    res = _uncompress_to(buf, cap, max_planes, max_stripe_out, trace, mine)
    if res[0] == OK:
        events.update(mine)
    return res


def _uncompress_to(buf, cap, max_planes, max_stripe_out, trace, events):
    buf = bytes(buf)
    size = len(buf)
    if size == 0:
        return E_EMPTY, b""
    if not buf[0] & X_STRIPE:
        t = []
        st, out = _piece(buf, 0, size, cap, t, events)
        if trace is not None and st == OK:
            trace.extend(t)
        return st, out
    nb, ulen = var_get(buf, 1, size)
    meta = 1 + nb
    if meta >= size:
        return E_TRUNCATED, b""
    N = buf[meta]
    meta += 1
    if cap is None:
        if ulen >= INT_MAX:
            return E_SIZE, b""
    elif ulen != cap:
        return E_CAPACITY, b""
    if N > max_planes or (max_stripe_out is not None and ulen > max_stripe_out):
        return E_UNSUPPORTED, b""
    if N == 0 and ulen:
        return E_SIZE, b""                                   # (the reference's unstripe does not return from this)
    clen, tot = [], 0
    for i in range(N):
        nb, c = var_get(buf, meta, size)
        meta += nb
        tot += c
        if c > size:
            return E_TRUNCATED, b""
        if c < 1:
            return E_SIZE, b""
        clen.append(c)
    if meta + tot > size:
        return E_TRUNCATED, b""
    size = meta + tot
    planes, t = [], []
    for i in range(N):
        want = ulen // N + (ulen % N > i)
        if buf[meta] & X_STRIPE:
            return E_UNSUPPORTED, b""                        # a plane that is itself a stripe stream: not supported
        st, p = _piece(buf, meta, size, want, t, events)
        if st:
            return st, b""
        if len(p) != want:
            return E_SIZE, b""
        planes.append(p)
        meta += clen[i]
    out = bytearray(ulen)
    for j in range(N):
        out[j::N] = planes[j]
    if trace is not None:
        trace.extend(t)                                      # (a block that is refused counts none of its planes)
    return OK, bytes(out)


def uncompress(buf):
    return uncompress_to(buf, None)


def fixtures():
    """[(name, text name, order, stream)] of the reference's 28 streams (one stream a file, nothing around it)"""
    out = []
    for fn in sorted(os.listdir(GOLDEN)):
        base, _, order = fn.rpartition(".")
        if order.isdigit():
            out.append((fn, base, int(order), open(os.path.join(GOLDEN, fn), "rb").read()))
    return out


def text(name):
    return open(os.path.join(HERE, "golden", "dat", name + ".nl"), "rb").read()
