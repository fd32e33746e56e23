"""A Python restatement of htscodecs' quality codec (fqzcomp_qual.c on c_simple_model.h and c_range_coder.h, whose
restatement is arith_model.py's): read_array and store_array, the parameter reader and writer, fqz_update_ctx, the
decode loop of uncompress_block_fqz2f and the encode loop of compress_block_fqz2f under caller-supplied parameters.  It
is the checker of the fqz tests and is itself pinned by the reference-made files of tests/golden/fqzcomp
(test_fqz_cpu.py), by nothing made from itself.

decompress gives (status, bytes, lengths): the statuses are those of htscodecs_amd/csrc/r4x16_fqz_parse.h and of the
decode loop of r4x16_fqz.hip - 0 where the reference returns a buffer, another code where it returns NULL or, for the
cases DESIGN 5 names, where the reference is undefined (`undefined(stream)` tells the two apart)."""
import os
import struct

from arith_model import Model, Decoder, Encoder, var_put, var_get, MAX_FREQ, STEP

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fqzcomp")

OK, E_CAPACITY, E_TRUNCATED, E_TABLE, E_SIZE, E_UNSUPPORTED, E_CONTEXT, E_EMPTY = 0, 1, 2, 3, 5, 6, 7, 9
GFLAG_MULTI_PARAM, GFLAG_HAVE_STAB, GFLAG_DO_REV = 1, 2, 4
PFLAG_DO_DEDUP, PFLAG_DO_LEN, PFLAG_DO_SEL, PFLAG_HAVE_QMAP, PFLAG_HAVE_PTAB, PFLAG_HAVE_DTAB, PFLAG_HAVE_QTAB = 2, 4, 8, 16, 32, 64, 128
FQZ_VERS = 5
FREVERSE = 16
LDS_PARAMS = 8                      # r4x16_fqz.hip FQ_LDS_PARAMS: parameter blocks whose tables a decode wave holds in LDS
KINDS = ("streams", "tab_lds", "tab_global", "do_rev", "multi_param", "dup")


# ---- store_array / read_array (:106-194) -------------------------------------------------------------------------
def store_array(array):
    size, tmp, i, j = len(array), [], 0, 0
    while i < size:
        run = i
        while i < size and array[i] == j:
            i += 1
        run = i - run
        while True:
            r = min(255, run)
            tmp.append(r)
            run -= r
            if r != 255:
                break
        j += 1
    out, last, j = [], -1, 0
    while j < len(tmp):
        v = tmp[j]
        j += 1
        out.append(v)
        if v == last:
            n = j
            while j < len(tmp) and tmp[j] == last:
                j += 1
            out.append(j - n)
        else:
            last = v
    assert all(v < 256 for v in out)
    return bytes(out)


def read_array(buf, pos, avail, size):
    """(bytes consumed or -1, the array): -1 is one of the undefined cases, the array is then partly written"""
    size = min(1024, size)
    R, i, z, last = [], 0, 0, -1
    while z < size and i < avail:
        run = buf[pos + i]
        R.append(run)
        z += run
        if run == last:
            if i + 1 >= avail:
                return -1, None
            i += 1
            copy = buf[pos + i]
            z += run * copy
            while copy and z < size and len(R) < 1024:
                copy -= 1
                R.append(run)
        if len(R) >= 1024:
            return -1, None
        last = run
        i += 1
    nb, array, zi, val = i, [], 0, 0
    while len(array) < size:
        if zi >= len(R):
            return -1, None
        run_len = 0
        while True:
            part = R[zi]
            zi += 1
            run_len += part
            if not (part == 255 and zi < len(R)):
                break
        if part == 255:
            return -1, None
        array.extend([val] * min(run_len, size - len(array)))
        val += 1
    return nb, array


# ---- the parameter reader (:1162-1283) ---------------------------------------------------------------------------
class Param:
    __slots__ = ("context", "pflags", "max_sym", "qbits", "qshift", "qloc", "sloc", "ploc", "dloc", "qmask", "qmap", "qtab", "ptab", "dtab")


class Header:
    __slots__ = ("out_size", "hdr", "gflags", "nparam", "max_sel", "max_sym", "stab", "p")


def parse(buf, events=None):
    """(status, Header): the walk of r4x16_fqz_parse.h.  events: a list that takes the refusal site or undefined rule."""
    def note(e):
        if events is not None:
            events.append(e)
    size = len(buf)
    h = Header()
    h.out_size = h.hdr = h.gflags = h.nparam = h.max_sel = h.max_sym = 0
    if size == 0:
        note("refuse:empty")
        return E_EMPTY, h
    q, h.out_size = var_get(buf, 0, size)
    if size - q < 10:
        note("refuse:short")
        return E_TRUNCATED, h
    if buf[q] != FQZ_VERS:
        note("refuse:version")
        return E_UNSUPPORTED, h
    gflags = buf[q + 1]
    q += 2
    nparam = 1
    if gflags & GFLAG_MULTI_PARAM:
        nparam = buf[q]
        q += 1
    if nparam == 0:
        note("refuse:nparam")
        return E_SIZE, h
    max_sel = nparam if nparam > 1 else 0
    if gflags & GFLAG_HAVE_STAB:
        max_sel = buf[q]
        q += 1
        r, stab = read_array(buf, q, size - q, 256)
        if r < 0:
            note("undefined:read_array")
            return E_TABLE, h
        q += r
    else:
        stab = [min(i, nparam - 1) for i in range(256)]
    h.p = []
    max_sym = 0
    for _ in range(nparam):
        avail = size - q
        if avail < 7:
            note("refuse:param_short")
            return E_TRUNCATED, h
        pm = Param()
        pm.context = buf[q] | (buf[q + 1] << 8)
        pm.pflags, pm.max_sym = buf[q + 2], buf[q + 3]
        pm.qbits, pm.qshift = buf[q + 4] >> 4, buf[q + 4] & 15
        pm.qloc, pm.sloc = buf[q + 5] >> 4, buf[q + 5] & 15
        pm.ploc, pm.dloc = buf[q + 6] >> 4, buf[q + 6] & 15
        pm.qmask = (1 << pm.qbits) - 1
        idx = 7
        if (pm.pflags & PFLAG_DO_SEL) and max_sel == 0:
            note("undefined:sel_model")
            return E_TABLE, h
        if pm.pflags & PFLAG_HAVE_QMAP:
            if idx + pm.max_sym > avail:
                note("refuse:qmap")
                return E_TRUNCATED, h
            pm.qmap = list(buf[q + idx:q + idx + pm.max_sym]) + [0xff] * (256 - pm.max_sym)     # (unsigned char)INT_MAX
            idx += pm.max_sym
        else:
            pm.qmap = list(range(256))
        tabs = []
        for flag, n, on in ((PFLAG_HAVE_QTAB, 256, pm.qbits != 0), (PFLAG_HAVE_PTAB, 1024, True), (PFLAG_HAVE_DTAB, 256, True)):
            if on and (pm.pflags & flag):
                r, t = read_array(buf, q + idx, avail - idx, n)
                if r < 0:
                    note("undefined:read_array")
                    return E_TABLE, h
                idx += r
            else:
                t = list(range(256)) if flag == PFLAG_HAVE_QTAB else [0] * n
            tabs.append(t)
        pm.qtab = tabs[0]
        pm.ptab = [(v << pm.ploc) & 0xffff for v in tabs[1]]
        pm.dtab = [(v << pm.dloc) & 0xffff for v in tabs[2]]
        q += idx
        max_sym = max(max_sym, pm.max_sym)
        h.p.append(pm)
    h.hdr, h.gflags, h.nparam, h.max_sel, h.max_sym, h.stab = q, gflags, nparam, max_sel, max_sym, stab
    return OK, h


def flat_tables(h):
    """the tables of an accepted header as r4x16_fqz_parse.h's sink lays them out: the selector table as 16-bit values,
    then per parameter block 16 bytes of scalars, qmap as bytes, qtab, ptab << ploc and dtab << dloc as 16-bit values"""
    out = struct.pack("<256H", *[v & 0xffff for v in h.stab])
    for pm in h.p:
        out += struct.pack("<HHBBBBB7x", pm.context, pm.qmask, pm.pflags, pm.qshift, pm.qloc, pm.sloc, pm.max_sym)
        out += bytes(pm.qmap) + struct.pack("<256H", *[v & 0xffff for v in pm.qtab])
        out += struct.pack("<1024H", *pm.ptab) + struct.pack("<256H", *pm.dtab)
    return out


def undefined(buf):
    """whether the stream is one of the cases where the reference is undefined and this library refuses"""
    ev = []
    parse(buf, ev)
    return any(e.startswith("undefined:") for e in ev)


# ---- the decoder (:1286-1490) ------------------------------------------------------------------------------------
def _symbol(rc, m, ev, what):
    """Decoder.symbol with the census: halvings, swaps, swaps across a lane boundary (a lane holds four list positions),
    an entry left level with the neighbour before it"""
    if ev is None:
        return rc.symbol(m)
    tot, pos_before = m.tot, rc.pos
    before, order = list(m.F), list(m.S)
    sym = rc.symbol(m)
    halved = False
    if m.F == before:
        ev.append(what + ":no_update")                               # freq > MAX_FREQ, or the scan ran off the list
    else:
        halved = tot + STEP > MAX_FREQ
        i = m.S.index(sym)
        level = i > 0 and m.F[i] == m.F[i - 1]
        if halved:
            ev.append(what + ":halve")
            if level:                                                # level with its neighbour after the halving: it stays
                ev.append(what + ":halve_tie")
        if level and m.S == order:                                   # after any update, and no swap: `>` not `>=`
            ev.append(what + ":level")
    if m.S != order:
        i = order.index(sym)
        ev.append(what + ":swap")
        if halved:
            ev.append(what + ":halve_swap")                          # the step that halves the model also moves the entry up
        if i % 4 == 0:
            ev.append(what + ":swap_lane")
    if pos_before >= rc.end and m.F != before:
        ev.append("coder:dry")                                       # a symbol decoded with no input left
    return sym


def decompress(buf, cap=None, nlengths=None, events=None, route=None):
    """(status, bytes, lengths).  cap: the output's capacity (None: the stored size).  lengths: every record's length, or
    the first nlengths.  events: the census; route: a Counter that takes the route kinds (R4X16_FQZ_*) of the stream."""
    ev = events
    st, h = parse(buf, ev)
    if st != OK:
        return st, b"", []
    n = h.out_size
    if cap is not None and cap < n:
        if ev is not None:
            ev.append("refuse:capacity")
        return E_CAPACITY, b"", []
    if route is not None and n:                                      # a decode wave takes the stream, wherever it ends
        route.update({"streams": 1, "tab_lds" if h.nparam <= LDS_PARAMS else "tab_global": 1,
                      "do_rev": 1 if h.gflags & GFLAG_DO_REV else 0, "multi_param": 1 if h.nparam > 1 else 0})
    out = bytearray(n)
    qual = {}
    m_len = [Model(256) for _ in range(4)]
    m_rev, m_dup = Model(2), Model(2)
    m_sel = Model(h.max_sel + 1) if h.max_sel > 0 else None
    rc = Decoder(buf, h.hdr, len(buf))
    if ev is not None and rc.pos >= rc.end:
        ev.append("coder:never_starts")
    nsym = h.max_sym + 1
    have_stab, do_rev = h.gflags & GFLAG_HAVE_STAB, h.gflags & GFLAG_DO_REV
    pm = h.p[0]
    i = p = s = delta = prevq = qctx = last = last_len = 0
    first_len = True
    lengths, revs, dups = [], [], 0

    def fail(code, why):
        if ev is not None:
            ev.append("refuse:" + why)
        return code, b"", []
    while i < n:
        if p == 0:
            s = _symbol(rc, m_sel, ev, "sel") if pm.pflags & PFLAG_DO_SEL else 0
            x = h.stab[min(255, s)] if have_stab else s                   # (a symbol of a 256-entry model: the MIN never bites)
            if x >= h.nparam:
                return fail(E_CONTEXT, "param")
            if ev is not None and pm is not h.p[x]:
                ev.append("param:switch")
            pm = h.p[x]
            ln = last_len
            if not (pm.pflags & PFLAG_DO_LEN) or first_len:
                ln = 0
                for k in range(4):
                    ln |= _symbol(rc, m_len[k], ev, "len") << (8 * k)
                first_len = False
                last_len = ln
            elif ev is not None:
                ev.append("len:carried")
            if ln > n - i:
                return fail(E_SIZE, "len_remainder")
            if ln == 0:
                return fail(E_SIZE, "len_zero")
            lengths.append(ln)
            if do_rev:
                revs.append(_symbol(rc, m_rev, ev, "rev"))
            if (pm.pflags & PFLAG_DO_DEDUP) and _symbol(rc, m_dup, ev, "dup"):
                if ln > i:
                    return fail(E_SIZE, "dup_length")
                out[i:i + ln] = out[i - ln:i]
                if ev is not None:
                    ev.append("dup:taken")
                    if ln > 64:
                        ev.append("dup:wave")                        # the copy takes the wave a second trip
                    if len(lengths) > 1 and lengths[-2] != ln:
                        ev.append("dup:other_length")
                i += ln
                dups += 1
                continue
            p, delta, prevq, qctx = ln, 0, 0, 0
            last = pm.context
        m = qual.get(last)
        if m is None:
            m = qual[last] = Model(nsym)
            if ev is not None:
                ev.append("row:first")
        elif ev is not None:
            ev.append("row:revisit")
        Q = _symbol(rc, m, ev, "qual") & 0xff
        out[i] = pm.qmap[Q]
        if ev is not None and Q >= pm.max_sym and (pm.pflags & PFLAG_HAVE_QMAP):
            ev.append("qmap:beyond")
        i += 1
        qctx = ((qctx << pm.qshift) + pm.qtab[Q]) & 0xffffffff
        last = (qctx & pm.qmask) << pm.qloc
        if ev is not None:
            if p > 1023:
                ev.append("clamp:p")
            if delta > 255:
                ev.append("clamp:delta")
        last += pm.ptab[min(1023, p)] + pm.dtab[min(255, delta)] + (s << pm.sloc)
        if ev is not None and last > 0xffff:
            ev.append("ctx:wrap")
        last &= 0xffff
        delta += prevq != Q
        prevq = Q
        p -= 1
    if do_rev:
        at = 0
        for k, (ln, rev) in enumerate(zip(lengths, revs)):
            if rev:
                out[at:at + ln] = out[at:at + ln][::-1]
                if ev is not None:
                    ev.append("rev:odd" if ln & 1 else "rev:even")
                    ev.append("rev:wave" if ln > 32 else "rev:lane")    # the device's end pass: by the wave, by its lane
                    if k >= 64:
                        ev.append("rev:later_trip")                  # ... which takes 64 records a trip
            at += ln
        if ev is not None:
            for k in range(0, len(lengths) - 63, 64):
                if all(r and ln > 32 for ln, r in zip(lengths[k:k + 64], revs[k:k + 64])):
                    ev.append("rev:trip_all_wave")                   # a trip whose 64 records are all the wave's
    if route is not None and dups:
        route.update({"dup": 1})
    return OK, bytes(out), lengths if nlengths is None else lengths[:nlengths]


# ---- the encoder under given parameters (:696-752, :952-1154) ----------------------------------------------------
def gparams(params, gflags=0, max_sel=None, stab=None):
    """params: a list of dicts with context, pflags, max_sym, qbits, qshift, qloc, sloc, ploc, dloc, pbits, dbits and the
    tables qmap (forward: quality -> symbol or None), qtab, ptab, dtab (unshifted)"""
    nparam = len(params)
    if nparam > 1:
        gflags |= GFLAG_MULTI_PARAM
    if max_sel is None:
        max_sel = nparam if nparam > 1 else 0
    if stab is None:
        stab = [min(i, nparam - 1) for i in range(256)]
    return {"gflags": gflags, "nparam": nparam, "max_sel": max_sel, "stab": list(stab), "p": params,
            "max_sym": max(pm["max_sym"] for pm in params)}


def param(max_sym=255, context=0, qbits=8, qshift=4, qloc=0, sloc=14, ploc=8, dloc=12, pbits=0, pshift=0, dbits=0, dshift=0,
          do_sel=False, do_len=False, do_dedup=False, qmap_of=None, qtab=None):
    """a parameter block in the manner of fqz_pick_parameters: ptab = min(2^pbits - 1, i >> pshift), dtab likewise"""
    pm = {"context": context, "max_sym": max_sym, "qbits": qbits, "qshift": qshift, "qloc": qloc, "sloc": sloc, "ploc": ploc,
          "dloc": dloc, "pbits": pbits, "dbits": dbits}
    pm["ptab"] = [min((1 << pbits) - 1, i >> pshift) if pbits else 0 for i in range(1024)]
    pm["dtab"] = [min((1 << dbits) - 1, i >> dshift) if dbits else 0 for i in range(256)]
    pm["qtab"] = list(qtab) if qtab is not None else list(range(256))
    if qmap_of is not None:                                          # the qualities in use, ascending: symbol = rank
        pm["qmap"] = [None] * 256
        for j, q in enumerate(sorted(set(qmap_of))):
            pm["qmap"][q] = j
        pm["max_sym"] = len(set(qmap_of))
    else:
        pm["qmap"] = list(range(256))
    pm["pflags"] = ((PFLAG_HAVE_QTAB if qtab is not None else 0) | (PFLAG_HAVE_DTAB if dbits else 0) | (PFLAG_HAVE_PTAB if pbits else 0) |
                    (PFLAG_DO_SEL if do_sel else 0) | (PFLAG_DO_LEN if do_len else 0) | (PFLAG_DO_DEDUP if do_dedup else 0) |
                    (PFLAG_HAVE_QMAP if qmap_of is not None else 0))
    return pm


def store_parameters(gp):
    out = bytearray([FQZ_VERS, gp["gflags"]])
    if gp["gflags"] & GFLAG_MULTI_PARAM:
        out.append(gp["nparam"])
    if gp["gflags"] & GFLAG_HAVE_STAB:
        out.append(gp["max_sel"])
        out += store_array(gp["stab"])
    for pm in gp["p"]:
        out += bytes([pm["context"] & 0xff, pm["context"] >> 8, pm["pflags"], pm["max_sym"], (pm["qbits"] << 4) | pm["qshift"],
                      (pm["qloc"] << 4) | pm["sloc"], (pm["ploc"] << 4) | pm["dloc"]])
        if pm["pflags"] & PFLAG_HAVE_QMAP:
            out += bytes(q for q in range(256) if pm["qmap"][q] is not None)
        if pm["qbits"] and (pm["pflags"] & PFLAG_HAVE_QTAB):
            out += store_array(pm["qtab"])
        if pm["pbits"] and (pm["pflags"] & PFLAG_HAVE_PTAB):
            out += store_array(pm["ptab"])
        if pm["dbits"] and (pm["pflags"] & PFLAG_HAVE_DTAB):
            out += store_array(pm["dtab"])
    return bytes(out)


def compress(data, lens, flags, gp):
    """compress_block_fqz2f with the caller's parameters: flags[rec] holds FREVERSE and the selector << 16"""
    data = bytearray(data)
    n, nrec = len(data), len(lens)
    out = bytearray(var_put(n)) + store_parameters(gp)
    P = gp["p"]
    qmask = [(1 << pm["qbits"]) - 1 for pm in P]
    ptab = [[v << pm["ploc"] for v in pm["ptab"]] for pm in P]
    dtab = [[v << pm["dloc"] for v in pm["dtab"]] for pm in P]
    qual = {}
    m_len = [Model(256) for _ in range(4)]
    m_rev, m_dup = Model(2), Model(2)
    m_sel = Model(gp["max_sel"] + 1) if gp["max_sel"] > 0 else None
    nsym = gp["max_sym"] + 1
    rc = Encoder()

    def reverse():
        i = rec = 0
        while i < n:
            ln = lens[rec] if rec < nrec - 1 else n - i
            if flags[rec] & FREVERSE:
                data[i:i + ln] = data[i:i + ln][::-1]
            i += ln
            rec += 1
    if gp["gflags"] & GFLAG_DO_REV:
        reverse()
    x = 0
    i = rec = p = s = delta = prevq = qctx = last = last_len = 0
    first_len = True
    while i < n:
        if p == 0:
            pm = P[x]
            if (pm["pflags"] & PFLAG_DO_SEL) or (gp["gflags"] & GFLAG_MULTI_PARAM):
                s = flags[rec] >> 16 if rec < nrec else 0
                rc.symbol(m_sel, s)
            else:
                s = 0
            x = gp["stab"][s] if gp["gflags"] & GFLAG_HAVE_STAB else s
            pm = P[x]
            ln = lens[rec]
            if not (pm["pflags"] & PFLAG_DO_LEN) or first_len:
                for k in range(4):
                    rc.symbol(m_len[k], (ln >> (8 * k)) & 0xff)
                first_len = False
            if gp["gflags"] & GFLAG_DO_REV:
                rc.symbol(m_rev, 1 if flags[rec] & FREVERSE else 0)
            rec += 1
            p, delta, qctx, prevq = ln, 0, 0, 0
            last = pm["context"]
            if pm["pflags"] & PFLAG_DO_DEDUP:
                if i and ln == last_len and data[i - last_len:i] == data[i:i + ln]:
                    rc.symbol(m_dup, 1)
                    i += ln
                    p = 0
                    continue
                rc.symbol(m_dup, 0)
                last_len = ln
        pm = P[x]
        qm = pm["qmap"][data[i]]
        m = qual.get(last)
        if m is None:
            m = qual[last] = Model(nsym)
        rc.symbol(m, qm)
        qctx = ((qctx << pm["qshift"]) + pm["qtab"][qm]) & 0xffffffff
        last = ((qctx & qmask[x]) << pm["qloc"]) + ptab[x][min(1023, p)] + dtab[x][min(255, delta)] + (s << pm["sloc"])
        last &= 0xffff
        delta += prevq != qm
        prevq = qm
        p -= 1
        i += 1
    return bytes(out) + rc.finish()


# ---- the committed vectors ---------------------------------------------------------------------------------------
def text(name):
    with open(os.path.join(HERE, "golden", "dat", name + ".nl"), "rb") as f:
        return f.read()


def fixtures():
    """[(file name, text name, the stream, the qualities, the record lengths)] of the reference's 16 streams.  The
    qualities are the text less 33 (the reference's test program takes the ASCII offset off before it compresses); the
    record lengths are the text's line lengths, kept in NAME.lens since the .nl texts carry no newlines."""
    res = []
    for base in ("q4", "q8", "q40+dir", "qvar"):
        want = bytes((c - 33) & 0xff for c in text(base))
        with open(os.path.join(GOLDEN, base + ".lens")) as f:
            lens = [int(v) for v in f.read().split()]
        assert sum(lens) == len(want)
        for k in range(4):
            fn = "%s.%d" % (base, k)
            with open(os.path.join(GOLDEN, fn), "rb") as f:
                res.append((fn, base, f.read(), want, lens))
    return res


_vectors = {}


def vectors(fn):
    """a reference-made container of tests/golden/fqzcomp (its README): (inputs, damaged).  inputs: [(name, data or None,
    lens, flags, stream, size, SHA-256 or None)]; damaged: [(stream, answer)] with answer None where the reference returns
    NULL, else (length, records, SHA-256)."""
    if fn not in _vectors:
        with open(os.path.join(GOLDEN, fn), "rb") as f:
            b = f.read()
        assert b[:8] == b"FQEDGE1\n"
        pos = 8

        def u32():
            nonlocal pos
            pos += 4
            return struct.unpack_from("<I", b, pos - 4)[0]

        def blob(n):
            nonlocal pos
            pos += n
            return b[pos - n:pos]
        inputs, damaged = [], []
        for _ in range(u32()):
            name = blob(struct.unpack("<H", blob(2))[0]).decode()
            nrec = u32()
            lens = list(struct.unpack("<%dI" % nrec, blob(4 * nrec)))
            flags = list(struct.unpack("<%dI" % nrec, blob(4 * nrec)))
            stream = blob(u32())
            size = u32()
            stored = blob(1)[0]
            data = blob(size) if stored else None
            digest = None if stored else blob(32)
            inputs.append((name, data, lens, flags, stream, size, digest))
        for _ in range(u32()):
            stream = blob(u32())
            if blob(1)[0]:
                ln, nrec = u32(), u32()
                damaged.append((stream, (ln, nrec, blob(32).hex())))
            else:
                damaged.append((stream, None))
        assert pos == len(b)
        _vectors[fn] = (inputs, damaged)
    return _vectors[fn]


def edge():
    """edge.bin: the header's and the loop's edges, streams of up to 1,000 records"""
    return vectors("edge.bin")


def records():
    """records.bin: streams of thousands of records - the per-record models past their halvings, the end pass past its
    first trip"""
    return vectors("records.bin")


def model_refused():
    """streams the model constructs for the refusal sites of the header walk, two each: [(stream, site)]"""
    base = compress(bytes([1, 2, 3, 2] * 10), [40], [0], gparams([param(max_sym=8, qbits=4, qshift=2, qmap_of=[1, 2, 3])]))
    q = var_get(base, 0, len(base))[0]
    res = [(b"", "empty"), (b"", "empty"), (base[:q + 9], "short"), (base[:3], "short")]
    for v in (4, 6):
        b = bytearray(base)
        b[q] = v
        res.append((bytes(b), "version"))
    for pad in (b"", b"\x01"):                                       # nparam = 0, with and without a selector table behind it
        b = bytearray(base)
        b[q + 1] |= GFLAG_MULTI_PARAM
        res.append((bytes(b[:q + 2]) + b"\x00" + pad + bytes(b[q + 2:]), "nparam"))
    for cut in (3, 6):                                               # a second parameter block of fewer than seven bytes
        b = bytearray(base)
        b[q + 1] |= GFLAG_MULTI_PARAM
        hdr = parse(base)[1].hdr
        res.append((bytes(b[:q + 2]) + b"\x02" + bytes(b[q + 2:hdr]) + bytes(cut), "param_short"))
    for n in (5, 200):                                               # a qmap that runs past the end
        b = bytearray(base[:q + 12])
        b[q + 5] = n
        res.append((bytes(b), "qmap"))
    for s, site in res:
        ev = []
        assert parse(s, ev)[0] != OK and ev == ["refuse:" + site], (site, ev)
    return res


def model_undefined():
    """streams the model constructs for the undefined rules of DESIGN 5: the library must refuse each"""
    res = []
    base = compress(bytes([3, 4, 5, 4] * 20), [40, 40], [0, 0], gparams([param(max_sym=8, qbits=4, qshift=2, pbits=3, pshift=2, dbits=2)]))
    st, h = parse(base)
    assert st == OK
    q = var_get(base, 0, len(base))[0]
    # PFLAG_DO_SEL without a selector model
    b = bytearray(base)
    b[q + 4] |= PFLAG_DO_SEL
    res.append(bytes(b))
    # the same behind a selector table that says max_sel = 0
    b[q + 1] |= GFLAG_HAVE_STAB
    res.append(bytes(b[:q + 2]) + bytes([0]) + store_array([0] * 256) + bytes(b[q + 2:]))
    # a ptab whose run lengths do not fill the table: the first run claims everything, then the stream ends
    res.append(base[:q + 9] + bytes([0, 0]))
    # a table that starts at the end of the stream (a qmap of one byte in front of it: the stream keeps its ten bytes)
    b = bytearray(base[:q + 9] + b"\x03")
    b[q + 4] |= PFLAG_HAVE_QMAP
    b[q + 5] = 1
    res.append(bytes(b))
    # a selector table that ends inside a chain of 255s
    b = bytearray(base)
    b[q + 1] |= GFLAG_HAVE_STAB
    res.append(bytes(b[:q + 2]) + bytes([1, 255, 255, 250]) + bytes(b[q + 2:]))
    for s in res:
        assert undefined(s), s.hex()
    return res
