"""What the tests of fqzcomp_qual encoding share (test_fqz_enc_cpu.py, test_gpu_fqz_enc.py): the encode loop of
compress_block_fqz2f (fqzcomp_qual.c:952-1154) under PARAMETER BYTES - what a stream holds between its size and the range
coder's bytes, the parameter format of the library's encode calls - with the event census, the verdict the device's front
pass gives a block, and the lists of inputs the GPU tests encode.

fqz_model.py (pinned to the reference's streams by test_fqz_cpu.py) is not edited: its header walk reads the parameter
bytes, its Model and arith_model's Encoder code the symbols.  test_fqz_enc_cpu.py holds this loop to fqz_model.compress
and to the reference's streams.  Everything is seeded; nothing here needs a GPU.

Events:
  carry, ff_pending, ff_flush_plain, ff_flush_carry, ff_run2, shift2   the range coder's, as arith_enc_model.py counts them
  halve:qual / halve:len / halve:sel / halve:rev / halve:dup            a symbol whose update halves that model
  halve_tie:qual    ... and leaves the coded entry level with the one before it (no swap: `>` not `>=`)
  dup:taken         a record coded as a duplicate of the bytes before it
  len:carried       a record whose length is not coded (PFLAG_DO_LEN behind the first)
  tab_global        a stream with more than eight parameter blocks: the tables are read from the arena
  tab_lds           the others
  param:switch      a record whose parameter block is not the one before"""
import collections
import random

import arith_model as A
import fqz_model as M

KINDS = ("streams", "tab_lds", "tab_global", "do_rev", "multi_param", "dup")
PAD = 9                             # r4x16_fqz_enc.hip FQE_PAD: the bytes a stream has at least behind its parameters


class CountingEncoder(A.Encoder):
    def __init__(self, events):
        super().__init__()
        self.ev = events
        self.shifts = 0

    def _count(self, what):
        if self.ev is not None:
            self.ev[what] += 1

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

    def coded(self, m, sym, what):
        self.shifts = 0
        i = m.S.index(sym)
        if (self.low + sum(m.F[:i]) * (self.range // m.tot)) > A.M32:
            self._count("carry")
        halved = m.tot + A.STEP > A.MAX_FREQ
        if halved:
            self._count("halve:" + what)
        self.symbol(m, sym)
        k = m.S.index(sym)
        if halved and k > 0 and m.F[k] == m.F[k - 1]:
            self._count("halve_tie:" + what)                         # level with its neighbour after the halving: it stays
        assert self.shifts <= 2                                      # the capacity rule's premise
        if self.shifts == 2:
            self._count("shift2")


def parse_params(params):
    """(status, Header) of parameter bytes, as r4x16_fqz_enc.hip's fqe_parse walks them: a size byte of 0 in front, nine
    zero bytes behind, and the walk must end where the bytes end"""
    st, h = M.parse(b"\x00" + bytes(params) + bytes(PAD))
    if st == M.OK and h.hdr != len(params) + 1:
        st = M.E_TRUNCATED if h.hdr > len(params) + 1 else M.E_UNSUPPORTED
    if st == M.OK and (h.gflags & M.GFLAG_MULTI_PARAM) and h.max_sel == 0:
        st = M.E_TABLE
    return st, h


def params_of(stream):
    """the parameter bytes of a stream: between the size and the range coder's bytes"""
    st, h = M.parse(stream)
    assert st == M.OK
    q = A.var_get(stream, 0, len(stream))[0]
    return stream[q:h.hdr]


def inverse(pm, max_sym):
    """quality -> symbol of a parsed parameter block, None where the reference is undefined"""
    inv = [None] * 256
    if pm.pflags & M.PFLAG_HAVE_QMAP:
        for sym in range(pm.max_sym):
            inv[pm.qmap[sym]] = sym
    else:
        for q in range(max_sym + 1):
            inv[q] = q
    return inv


def verdict(data, lens, flags, params, max_sym_limit=255):
    """the status k_fqe_front gives the block (capacity aside)"""
    st, h = parse_params(params)
    if st != M.OK:
        return st
    if h.max_sym > max_sym_limit:
        return M.E_UNSUPPORTED
    n = len(data)
    if n == 0:
        return M.OK
    if not lens or any(v == 0 for v in lens) or sum(lens) != n:
        return M.E_SIZE
    uses_sel = bool(h.gflags & M.GFLAG_MULTI_PARAM) or bool(h.p[0].pflags & M.PFLAG_DO_SEL)
    xs = []
    for f in flags:
        s = f >> 16 if uses_sel else 0
        if uses_sel and s > h.max_sel:
            return M.E_CONTEXT
        x = h.stab[min(s, 255)] if h.gflags & M.GFLAG_HAVE_STAB else s
        if x >= h.nparam:
            return M.E_CONTEXT
        xs.append(x)
    invs = [inverse(pm, h.max_sym) for pm in h.p]
    at = 0
    for ln, x in zip(lens, xs):
        if any(invs[x][q] is None for q in data[at:at + ln]):
            return M.E_CONTEXT
        at += ln
    return M.OK


def compress(data, lens, flags, params, events=None, route=None):
    """compress_block_fqz2f under parameter bytes: flags[rec] holds FREVERSE (16) and the selector << 16.  The block must
    have verdict 0.  events: a Counter that takes the census; route: a Counter that takes the route kinds."""
    st, h = parse_params(params)
    assert st == M.OK, st
    ev = events
    data = bytearray(data)
    n, nrec = len(data), len(lens)
    out = bytearray(A.var_put(n)) + bytes(params)
    if n and route is not None:
        route.update({"streams": 1, "tab_lds" if h.nparam <= M.LDS_PARAMS else "tab_global": 1,
                      "do_rev": 1 if h.gflags & M.GFLAG_DO_REV else 0, "multi_param": 1 if h.nparam > 1 else 0})
    if n and ev is not None:
        ev["tab_lds" if h.nparam <= M.LDS_PARAMS else "tab_global"] += 1
    do_rev, have_stab = h.gflags & M.GFLAG_DO_REV, h.gflags & M.GFLAG_HAVE_STAB
    if do_rev:
        at = 0
        for rec in range(nrec):
            ln = lens[rec] if rec < nrec - 1 else n - at
            if flags[rec] & M.FREVERSE:
                data[at:at + ln] = data[at:at + ln][::-1]
            at += ln
    invs = [inverse(pm, h.max_sym) for pm in h.p]
    qual = {}
    m_len = [A.Model(256) for _ in range(4)]
    m_rev, m_dup = A.Model(2), A.Model(2)
    m_sel = A.Model(h.max_sel + 1) if h.max_sel > 0 else None
    nsym = h.max_sym + 1
    rc = CountingEncoder(ev)
    uses_sel = bool(h.gflags & M.GFLAG_MULTI_PARAM) or bool(h.p[0].pflags & M.PFLAG_DO_SEL)
    pm, x = h.p[0], 0
    i = rec = p = s = delta = prevq = qctx = last = last_len = dups = 0
    first_len = True
    while i < n:
        if p == 0:
            s = 0
            if uses_sel:
                s = flags[rec] >> 16
                rc.coded(m_sel, s, "sel")
            nx = h.stab[s] if have_stab else s
            if ev is not None and nx != x:
                ev["param:switch"] += 1
            x = nx
            pm = h.p[x]
            ln = lens[rec]
            if not (pm.pflags & M.PFLAG_DO_LEN) or first_len:
                for k in range(4):
                    rc.coded(m_len[k], (ln >> (8 * k)) & 0xff, "len")
                first_len = False
            elif ev is not None:
                ev["len:carried"] += 1
            if do_rev:
                rc.coded(m_rev, 1 if flags[rec] & M.FREVERSE else 0, "rev")
            rec += 1
            p, delta, qctx, prevq = ln, 0, 0, 0
            last = pm.context
            if pm.pflags & M.PFLAG_DO_DEDUP:
                if i and ln == last_len and data[i - last_len:i] == data[i:i + ln]:
                    rc.coded(m_dup, 1, "dup")
                    if ev is not None:
                        ev["dup:taken"] += 1
                    i += ln
                    p = 0
                    dups += 1
                    continue
                rc.coded(m_dup, 0, "dup")
                last_len = ln
        qm = invs[x][data[i]]
        m = qual.get(last)
        if m is None:
            m = qual[last] = A.Model(nsym)
        rc.coded(m, qm, "qual")
        qctx = ((qctx << pm.qshift) + pm.qtab[qm]) & 0xffffffff
        last = ((qctx & pm.qmask) << pm.qloc) + pm.ptab[min(1023, p)] + pm.dtab[min(255, delta)] + (s << pm.sloc)
        last &= 0xffff
        delta += prevq != qm
        prevq = qm
        p -= 1
        i += 1
    if route is not None and dups:
        route.update({"dup": 1})
    return bytes(out) + rc.finish()


def cap(size, nrec, params_size):
    """rans4x16_hip_fqz_compress_cap: varint 5, the parameters, two bytes a symbol, seven symbols a record beside its
    qualities, five to finish"""
    return min(0xffffffff, 5 + params_size + 2 * (size + 7 * nrec) + 5)


# ---- the inputs the GPU tests encode -----------------------------------------------------------------------------
def r2_flags():
    """the READ2 flags of q40+dir (tests/golden/fqzcomp/README.enc.md): FQZ_FREAD2 = 128 where the line says 1"""
    import os
    with open(os.path.join(M.GOLDEN, "q40+dir.r2")) as f:
        return [128 * int(v) for v in f.read().split()]


def fixture_slices():
    """[(file name, strat, the reference's stream, qualities, lens, flags)] of the 16 streams: vers 4, strat = suffix"""
    res = []
    for fn, base, stream, want, lens in M.fixtures():
        flags = r2_flags() if base == "q40+dir" else [0] * len(lens)
        res.append((fn, int(fn.rsplit(".", 1)[1]), stream, want, list(lens), flags))
    return res


def kept_vectors():
    """[(name, data, lens, flags, the reference's stream)] of edge.bin and records.bin: the inputs whose bytes are kept"""
    res = []
    for which, (inputs, _) in (("edge", M.edge()), ("records", M.records())):
        for name, data, lens, flags, stream, size, digest in inputs:
            if data is not None:
                res.append((which + ":" + name, data, list(lens), list(flags), stream))
    return res


_hashed = []


def hashed_vectors():
    """[(name, data, lens, flags, the reference's stream)] of edge.bin and records.bin: the inputs kept as a SHA-256 (those
    above 4 KiB - the tie after a halving, a record of 70,000 bytes, the slices of thousands of records).  The bytes are
    what fqz_model.decompress makes of the reference's stream, held to the file's digest and record lengths."""
    if not _hashed:
        import hashlib
        for which, (inputs, _) in (("edge", M.edge()), ("records", M.records())):
            for name, data, lens, flags, stream, size, digest in inputs:
                if data is None:
                    st, out, got = M.decompress(stream)
                    assert st == M.OK and len(out) == size and hashlib.sha256(out).digest() == digest and got == list(lens), name
                    _hashed.append((which + ":" + name, out, list(lens), list(flags), stream))
    return _hashed


_census_slice = []


def census_slice(seed=9):
    """(data, lens, flags, params): 8,400 records of 1 .. 4 bytes under GFLAG_DO_REV and two parameter blocks that both
    code selectors and duplicates and never carry a length - the `len`, `sel`, `revcomp` and `dup` models add 16 a record
    and halve above 65,519, at record 4,080 or so and again near 8,170.  Five qualities: duplicates come by themselves."""
    if not _census_slice:
        rng = random.Random(seed)
        pm = [M.param(max_sym=4, qbits=4, qshift=2, pbits=2, pshift=0, dbits=2, sloc=14, ploc=8, dloc=12, do_sel=True, do_dedup=True)
              for _ in range(2)]
        pm[1]["context"] = 0x100
        params = M.store_parameters(M.gparams(pm, gflags=M.GFLAG_DO_REV))
        lens = [rng.choice((1, 1, 2, 2, 3, 4)) for _ in range(8400)]
        flags = [(16 if rng.random() < 0.4 else 0) | ((1 if rng.random() < 0.2 else 0) << 16) for _ in lens]
        data = bytes(rng.choice((0, 1, 1, 2, 3, 3, 3, 4)) for _ in range(sum(lens)))
        _census_slice.append((data, lens, flags, params))
    return _census_slice[0]


def drop_in_case(seed=20):
    """a few hundred short records (1, 2, 31 .. 33, 63 .. 65 bytes) with mixed FQZ_FREVERSE flags, for vers 3"""
    rng = random.Random(seed)
    lens = [rng.choice((1, 2, 31, 32, 33, 63, 64, 65)) for _ in range(300)]
    flags = [16 if rng.random() < 0.4 else 0 for _ in lens]
    data = bytearray()
    for ln in lens:
        q = rng.randrange(20, 40)
        for _ in range(ln):
            if rng.random() < 0.3:
                q = min(41, max(2, q + rng.choice((-3, -1, 1, 2))))
            data.append(q)
    return bytes(data), lens, flags
