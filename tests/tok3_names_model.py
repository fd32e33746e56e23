"""Python model of the tok3 name decoder (htscodecs tokenise_name3.c:1018-1189, decode_name, and the loop around it at
:1671-1689) as include/rans4x16_hip.h part 2d states it - the stricter cases included - over the columns of one block.

  framing(cols, last_start, nreads, ..)  the verdict before any name is decoded (0 or a status)
  decode(cols, last_start, nreads, ..)   (status, bytes, name starts): the names NUL-separated; b"" and [] on failure
                                         (last_start None: without the size rule)
  history_units(cols)                    what the block claims of the call's history arena, in 16-byte units

cols is [(id, bytes)] with id = position << 4 | type, the type columns (type 0) included - tok3_model.columns() zipped
with the ids of its walk.  The model is pinned by the reference's own input files (tests/golden/names), not by the GPU.

Test infrastructure only: nothing in htscodecs_amd/ imports this module."""
import glob
import gzip
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = os.path.join(ROOT, "tests", "golden", "names")

OK, CAPACITY, TRUNCATED, SIZE, UNSUPPORTED = 0, 1, 2, 5, 6
N_TYPE, N_ALPHA, N_CHAR, N_DIGITS0, N_DZLEN, N_DUP, N_DIFF, N_DIGITS, N_DDELTA, N_DDELTA0, N_MATCH, N_NOP, N_END = range(13)
TOKENS = (N_ALPHA, N_CHAR, N_DIGITS0, N_DIGITS, N_DDELTA, N_DDELTA0, N_MATCH, N_NOP)
MAX_TOKENS = 128
MAX_COLUMN = 1 << 28          # a column of this many bytes or more: UNSUPPORTED (a string's place in its column takes 28 bits)
M32 = 0xFFFFFFFF


def names_files():
    """{'01': bytes, ..}: the reference's input files, one name per line (committed gzip-compressed: 75 KB for 487 KB)."""
    out = {}
    for p in sorted(glob.glob(os.path.join(NAMES, "*.names.gz"))):
        with gzip.open(p, "rb") as f:
            out[os.path.basename(p)[:-len(".names.gz")]] = f.read()
    return out


def uint32_var(v):
    """append_uint32_var (:279-315): decimal without leading zeros - and 0 gives no byte at all."""
    return str(v).encode() if v else b""


def uint32_fixed(v, width):
    """append_uint32_fixed (:263-277): `width` characters; a value that needs more has the quotient in its first
    character, truncated to 8 bits."""
    if width == 0:
        return b""
    p = 10 ** (width - 1)
    return bytes([(v // p + 48) & 0xFF]) + (b"%0*d" % (width - 1, v % p) if width > 1 else b"")


def _shape(cols):
    """(names the block holds, token positions it has)."""
    by = dict(cols)
    return len(by.get(0, b"")), max([cid >> 4 for cid, _ in cols] or [-1]) + 1


def framing(cols, last_start, nreads, max_names=1 << 30, max_tokens=MAX_TOKENS):
    count, npos = _shape(cols)
    if nreads == 0 or count > nreads or last_start >= 0x7FFFFFFF - 1024:
        return SIZE
    if npos > max_tokens or count > max_names:
        return UNSUPPORTED
    if any(len(d) >= MAX_COLUMN for _, d in cols):
        return UNSUPPORTED
    return OK


def history_units(cols):
    count, npos = _shape(cols)
    return count + (count * npos * 8 + 15) // 16


class _Cols:
    def __init__(self, cols):
        self.data = dict(cols)
        self.at = {cid: 0 for cid in self.data}

    def left(self, cid):
        return len(self.data[cid]) - self.at[cid] if cid in self.data else 0

    def take(self, cid, n):
        """n bytes of column cid, or None where it runs out (nothing is consumed then)."""
        if self.left(cid) < n:
            return None
        o = self.at[cid]
        self.at[cid] = o + n
        return self.data[cid][o:o + n]


def decode(cols, last_start, nreads, max_names=1 << 30, max_tokens=MAX_TOKENS):
    """last_start None: without the size rule - what the block decodes to, for tests that build blocks."""
    fail = lambda st: (st, b"", [])
    exact = last_start is not None
    if not exact:
        last_start = 0x7FFFFFFF - 1025
    st = framing(cols, last_start, nreads, max_names, max_tokens)
    if st != OK:
        return fail(st)
    count, npos = _shape(cols)
    c = _Cols(cols)
    out = bytearray()
    starts = []
    ends = []             # per name: its end position
    state = []            # per name: {position: (type, int, string)} - shared by a name and its duplicates
    for cnum in range(count):
        t0 = c.take(0, 1)[0]
        if t0 not in (N_DUP, N_DIFF):
            return fail(SIZE)
        d = c.take(t0, 4)
        if d is None:
            return fail(TRUNCATED)
        dist = int.from_bytes(d, "little")
        if dist > cnum or (t0 == N_DUP and dist == 0):
            return fail(SIZE)
        pnum = cnum - dist
        pend = ends[pnum] if dist else 0
        pst = state[pnum] if dist else {}
        name = bytearray()
        if t0 == N_DUP:
            mine, end = pst, pend
            for t in range(1, end):
                name += _render(pst[t])
        else:
            mine, end = {}, None
            for t in range(1, min(MAX_TOKENS, npos)):
                b = c.take(t << 4, 1)
                tok = b[0] if b is not None and b[0] in TOKENS else N_END
                if tok == N_END:
                    end = t
                    break
                if tok == N_CHAR:
                    v = c.take(t << 4 | N_CHAR, 1)
                    if v is None:
                        return fail(TRUNCATED)
                    mine[t] = (N_CHAR, v[0], b"")
                elif tok == N_ALPHA:
                    cid = t << 4 | N_ALPHA
                    if c.left(cid) == 0:
                        return fail(TRUNCATED)
                    z = c.data[cid].find(b"\0", c.at[cid])
                    if z < 0:
                        return fail(TRUNCATED)
                    mine[t] = (N_ALPHA, z - c.at[cid], c.take(cid, z - c.at[cid] + 1)[:-1])
                elif tok == N_DIGITS0:
                    vl = c.take(t << 4 | N_DZLEN, 1)
                    if vl is None:
                        return fail(TRUNCATED)
                    v = c.take(t << 4 | N_DIGITS0, 4)
                    if v is None:
                        return fail(TRUNCATED)
                    if vl[0] > 9:
                        return fail(SIZE)
                    mine[t] = (N_DIGITS0, int.from_bytes(v, "little"), vl[0])
                elif tok == N_DIGITS:
                    v = c.take(t << 4 | N_DIGITS, 4)
                    if v is None:
                        return fail(TRUNCATED)
                    mine[t] = (N_DIGITS, int.from_bytes(v, "little"), 0)
                elif tok in (N_DDELTA, N_DDELTA0):
                    if t >= pend:
                        return fail(SIZE)
                    v = c.take(t << 4 | tok, 1)
                    if v is None:
                        return fail(TRUNCATED)
                    kind = N_DIGITS if tok == N_DDELTA else N_DIGITS0
                    if pst[t][0] != kind:
                        return fail(SIZE)
                    mine[t] = (kind, (pst[t][1] + v[0]) & M32, pst[t][2])
                elif tok == N_MATCH:
                    if t >= pend or pst[t][0] == N_NOP:
                        return fail(SIZE)
                    mine[t] = pst[t]
                else:
                    mine[t] = (N_NOP, 0, 0)
                name += _render(mine[t])
            if end is None:
                return fail(SIZE)
        name += b"\0"
        if len(out) + len(name) > last_start:
            return fail(SIZE)
        starts.append(len(out))
        out += name
        ends.append(end)
        state.append(mine)
    if exact and len(out) != last_start:
        return fail(SIZE)
    return OK, bytes(out), starts


def _render(tok):
    kind, v, s = tok
    if kind == N_CHAR:
        return bytes([v & 0xFF])
    if kind == N_ALPHA:
        return s
    if kind == N_DIGITS:
        return uint32_var(v)
    if kind == N_DIGITS0:
        return uint32_fixed(v, s)
    return b""
