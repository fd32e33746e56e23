"""Python model of the tok3 column container in its arith flavour (use_arith = 1: htscodecs tokenise_name3.c with
arith_compress_to / arith_uncompress_to in place of the rANS calls, :1246-1321, and byte 8 set, :1511), composed of the
models the other tok3 and arith tests pin: tok3_model.walk (flag byte and stored size lie where rANS has them, so the walk
is the same once byte 8 is cleared), arith_model.uncompress_to, tok3_names_model.decode, arith_enc_model.compress and
tok3_model.frame.

Test infrastructure only: nothing in htscodecs_amd/ imports this module."""
import functools
import glob
import os

import arith_enc_model as AE
import arith_model as A
import tok3_model as M
import tok3_names_model as N

# tokenise_name3.c:1255-1259, the method rows of the levels 1-2, 3-4, 5-6, 7-8, 9
ROWS = {1: [0, 128], 3: [0, 200], 5: [0, 128, 201], 7: [0, 1, 129, 65, 193, 201], 9: [0, 1, 128, 129, 64, 65, 192, 193, 201]}


@functools.lru_cache(maxsize=None)
def fixtures():
    """((name, bytes), ..) of the 55 arith containers (*.names.11 .. *.names.19), sorted by name."""
    out = []
    for p in sorted(glob.glob(os.path.join(M.GOLDEN, "*.names.1[13579]"))):
        with open(p, "rb") as f:
            out.append((os.path.basename(p), f.read()))
    return tuple(out)


def level_of(name):
    """the reference's inner level 1..9 of a fixture: its suffix less the 10 that stands for use_arith"""
    return int(name.rsplit(".", 1)[1]) - 10


# the fixtures the model's frame reproduces byte for byte (the others hold, in near-constant columns, streams of the same
# lengths with other bytes - an older build's flush; all 55 decode to their names files)
BYTE_EXACT = tuple(n for n, _ in fixtures() if n.endswith((".17", ".19")))


def is_arith(buf):
    return len(buf) > 8 and buf[8] != 0


def cleared(buf):
    """the container with byte 8 (use_arith) cleared: what tok3_model.walk takes"""
    return bytes(buf[:8]) + b"\0" + bytes(buf[9:]) if len(buf) > 8 else bytes(buf)


def walk(buf, **kw):
    """The walk of either flavour (rans4x16_hip_tok3_scan_any): (Walk, use_arith)."""
    return M.walk(cleared(buf), **kw), int(is_arith(buf))


def decode_columns(buf, w, max_planes=4, max_stripe_out=None):
    """(status, [bytes of every column, type columns included]) of a walked arith container, as unpack_dev gives them: the
    status of the first plain column that fails to decode - the decoder's own, or SIZE for a column that decodes to another
    size than it claims - and no columns then.  The decoder is handed the REST OF THE CONTAINER from the stream's first
    byte with the claim as capacity, as tokenise_name3.c:1214 hands it: c_range_coder.h:64 starts to decode only if more
    than five bytes lie in front of the input's end, and a near-constant column's body is exactly five."""
    buf = bytes(buf)
    out = []
    for c in w.cols:
        if c["kind"] == M.PLAIN:
            st, d = A.uncompress_to(buf[c["stream_off"]:], c["size"], max_planes=max_planes, max_stripe_out=max_stripe_out)
            if st != A.OK:
                return st, None
            if len(d) != c["size"]:
                return M.SIZE, None
            out.append(d)
        elif c["kind"] == M.SYNTH:
            out.append(bytes([c["type"]]) + bytes([M.N_MATCH]) * (c["size"] - 1))
        else:
            out.append(out[c["src"]] if c["src"] is not None else b"")
    return M.OK, out


def columns(buf, w=None):
    """The bytes of every column of an arith container (type columns included), or None where a stream is refused."""
    if w is None:
        w = M.walk(cleared(buf))
    assert w.status == M.OK
    return decode_columns(buf, w)[1]


def names(buf):
    """decode_names of an arith container: (status, NUL-separated names)."""
    w = M.walk(cleared(buf))
    if w.status != M.OK:
        return w.status, b""
    st, cols = decode_columns(buf, w)
    if st != M.OK:
        return st, b""
    st, out, _ = N.decode([(c["id"], d) for c, d in zip(w.cols, cols)], w.last_start, w.nreads)
    return st, out


def frame(cols, methods, last_start, nreads):
    """encode_names' framing over cols = [(id, bytes)] with use_arith = 1: (container, [method per column])."""
    out, chosen = M.frame(AE.compress, cols, methods, last_start, nreads)
    return out[:8] + b"\1" + out[9:], chosen


def reframed(buf, methods):
    """A container's own described columns framed anew: what pack_dev gives for them."""
    w = M.walk(cleared(buf))
    cols = columns(buf, w)
    return frame([(cid, cols[i]) for cid, i in M.described(w)], methods, w.last_start, w.nreads)
