"""Python mirror of the reference interface (htscodecs/rANS_static4x16.h:41-50) on top of the
C ABI, plus the batch calls.  Same names and argument meaning as the C functions; errors come
back as ``None`` exactly where the C functions return NULL."""
import ctypes as C

import threading

import numpy as np

from . import lib as _lib


def rans_compress_bound_4x16(size, order):
    return _lib.load().rans_compress_bound_4x16(size, order)


def rans_compress_4x16(data, order):
    """bytes -> compressed bytes, or None (C: NULL).  rANS_static4x16pr.c:1347."""
    L = _lib.load()
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = L.rans_compress_bound_4x16(len(src), order)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_uint(cap)
    r = L.rans_compress_to_4x16(src.ctypes.data if len(src) else out.ctypes.data, len(src),
                                out.ctypes.data, C.byref(n), order)
    return out[:n.value].tobytes() if r else None


def rans_uncompress_4x16(comp, out_size=None):
    """compressed bytes -> bytes, or None.  out_size: capacity of the caller buffer (needed for
    X_NOSZ streams, rANS_static4x16pr.c:1456)."""
    L = _lib.load()
    src = np.frombuffer(bytes(comp), dtype=np.uint8)
    if out_size is None:
        n = C.c_uint(0)
        p = L.rans_uncompress_4x16(src.ctypes.data, len(src), C.byref(n))
        if not p:
            return None
        res = C.string_at(p, n.value)
        C.CDLL(None).free(C.c_void_p(p))
        return res
    out = np.empty(out_size + 1, dtype=np.uint8)
    n = C.c_uint(out_size)
    r = L.rans_uncompress_to_4x16(src.ctypes.data, len(src), out.ctypes.data, C.byref(n))
    return out[:n.value].tobytes() if r else None


# ---- rANS 4x8 (include/rans4x8_hip.h; htscodecs/rANS_static.h:41-44) ---------------------------------------

def rans_compress(data, order):
    """bytes -> rANS 4x8 stream, or None (C: NULL).  rANS_static.c:927."""
    L = _lib.load()
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    n = C.c_uint(0)
    dummy = np.zeros(1, dtype=np.uint8)
    p = L.rans_compress(src.ctypes.data if len(src) else dummy.ctypes.data, len(src), C.byref(n), order)
    if not p:
        return None
    res = C.string_at(p, n.value)
    C.CDLL(None).free(C.c_void_p(p))
    return res


def rans_uncompress(comp):
    """rANS 4x8 stream -> bytes, or None.  rANS_static.c:934."""
    L = _lib.load()
    src = np.frombuffer(bytes(comp) + bytes(16), dtype=np.uint8)
    n = C.c_uint(0)
    p = L.rans_uncompress(src.ctypes.data, len(comp), C.byref(n))
    if not p:
        return None
    res = C.string_at(p, n.value)
    C.CDLL(None).free(C.c_void_p(p))
    return res


class _HostArrays:
    """What every host-batch call takes - the blocks' pointers and sizes, an output buffer per block of its capacity, the
    sizes coming back, the statuses - and what it leaves.  caps: a capacity per block, or a function of a block's index and
    size that gives it."""

    def __init__(self, blocks, caps):
        n = self.n = len(blocks)
        self.srcs = [np.frombuffer(bytes(b), dtype=np.uint8) for b in blocks]
        capv = [int(caps(i, len(x))) for i, x in enumerate(self.srcs)] if callable(caps) else [int(c) for c in caps]
        self.outs = [np.empty(max(c, 1), dtype=np.uint8) for c in capv]
        self.dummy = np.zeros(1, dtype=np.uint8)
        self.in_p = (C.c_void_p * n)(*[(s.ctypes.data if len(s) else self.dummy.ctypes.data) for s in self.srcs])
        self.out_p = (C.c_void_p * n)(*[o.ctypes.data for o in self.outs])
        self.in_sz = (C.c_uint * n)(*[len(s) for s in self.srcs])
        self.out_sz = (C.c_uint * n)(*capv)
        self.status = (C.c_int * n)()

    def results(self):
        """(every block's bytes, None for a block that failed; the statuses)"""
        return [self.outs[i][:self.out_sz[i]].tobytes() if self.status[i] == 0 else None for i in range(self.n)], list(self.status)


def _library_allocates(blocks, call, who, ctx):
    """A host-batch compress call with out[i] == NULL: the library allocates exactly the result.  call(n, in_p, in_sz,
    out_p, out_sz, status) makes the library's call and returns its return code; the buffers are read and freed whatever
    that is.  Returns (the streams, None for a block that failed; the statuses)."""
    n = len(blocks)
    srcs = [np.frombuffer(bytes(b), dtype=np.uint8) for b in blocks]
    dummy = np.zeros(4, dtype=np.uint8)
    in_p = (C.c_void_p * n)(*[(s.ctypes.data if len(s) else dummy.ctypes.data) for s in srcs])
    in_sz = (C.c_uint * n)(*[len(s) for s in srcs])
    out_p = (C.c_void_p * n)()
    out_sz = (C.c_uint * n)()
    status = (C.c_int * n)()
    rc = call(n, in_p, in_sz, out_p, out_sz, status)
    outs = []
    for i in range(n):
        outs.append(C.string_at(out_p[i], out_sz[i]) if status[i] == 0 and out_p[i] else None)
        if out_p[i]:
            _free(out_p[i])
    if rc < 0:
        raise RuntimeError(who + ": " + ctx.error())
    return outs, list(status)


def _host_batch8(blocks, decode, orders=None, caps=None):
    ctx = _thread_ctx()
    L = ctx.L
    a = _HostArrays(blocks, caps if decode else lambda i, size: L.rans4x8_hip_compress_bound(size))
    if decode:
        rc = L.rans4x8_hip_uncompress_batch(ctx.h, a.n, a.in_p, a.in_sz, a.out_p, a.out_sz, a.status)
    else:
        rc = L.rans4x8_hip_compress_batch(ctx.h, a.n, a.in_p, a.in_sz, a.out_p, a.out_sz, _methods(orders), a.status)
    if rc < 0:
        raise RuntimeError("rans4x8 batch call failed: " + ctx.error())
    return a.results()


def compress_batch_4x8(blocks, orders):
    return _host_batch8(blocks, False, orders=orders)


def uncompress_batch_4x8(blocks, caps):
    return _host_batch8(blocks, True, caps=caps)


class _Ctx:
    def __init__(self, device=-1):
        self.L = _lib.load()
        self.h = self.L.rans4x16_hip_create(device)
        if not self.h:
            raise RuntimeError("rans4x16_hip_create failed: no usable HIP device (no CPU path exists)")

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.rans4x16_hip_destroy(self.h)
        except Exception:
            pass

    def error(self):
        return self.L.rans4x16_hip_last_error(self.h).decode()

    def set_option(self, name, value):
        if self.L.rans4x16_hip_set_option(self.h, name.encode(), int(value)) != 0:
            raise KeyError(f"unknown option {name!r}")

    def get_option(self, name):
        v = C.c_long(0)
        if self.L.rans4x16_hip_get_option(self.h, name.encode(), C.byref(v)) != 0:
            raise KeyError(f"unknown option {name!r}")
        return v.value

    def route_read(self, which, reset=True):
        """rans4x16_hip_route_read: {kind name: count} of `which` ("encode", "decode", "expand", "launch",
        "result", "names", "arith", "arith_enc", "fqz", "encode_body", "fqz_enc", "fqz_pick", "fqz_best", "best_any", "best_qual") since the last reset; needs option route_count = 1 while the calls run."""
        w = ROUTE_WHICH[which]
        kinds = ROUTE_KINDS[which]
        arr = (C.c_long * len(kinds))()
        rc = self.L.rans4x16_hip_route_read(self.h, w, arr, len(kinds), 1 if reset else 0)
        if rc != len(kinds):
            raise RuntimeError("route_read failed: " + self.error())
        return dict(zip(kinds, arr))


# include/rans4x16_hip.h: rans4x16_hip_route_read's lists and their kinds, in enum order
ROUTE_WHICH = {"encode": 0, "decode": 1, "expand": 2, "launch": 3, "result": 4, "names": 5, "arith": 6,
               "arith_enc": 7, "fqz": 8, "encode_body": 9, "fqz_enc": 10, "fqz_pick": 11, "fqz_best": 12, "best_any": 13,
               "best_qual": 14}
ROUTE_KINDS = {
    "encode": ("u16", "packed", "records", "packed_freq"),
    "decode": ("l1", "l2", "l3", "l4", "l5", "direct", "mid", "short_ring"),
    "expand": ("wave", "workgroup"),
    "launch": ("in_order", "side_by_side"),
    "result": ("in_slot", "dense", "gathered"),
    "names": ("enc_chunks", "dec_chunks", "uploaded", "refused"),
    "arith": ("o0", "o1_lds", "o1_global", "rle"),
    "arith_enc": ("o0", "o1_lds", "o1_global", "rle", "stored"),
    "fqz": ("streams", "tab_lds", "tab_global", "do_rev", "multi_param", "dup"),
    "encode_body": ("packed_affine",),
    "fqz_enc": ("streams", "tab_lds", "tab_global", "do_rev", "multi_param", "dup"),
    "fqz_pick": ("blocks", "sel", "split", "dedup", "undecided", "host"),
    "fqz_best": ("blocks", "candidates", "counted", "undecided", "refused"),
    "best_any": ("rans", "arith", "tie", "failed", "chunks"),
    "best_qual": ("blocks", "chunks", "rans", "arith", "fqz", "tie", "failed", "undecided"),
}

# include/rans4x16_hip.h part 2m: a method of the cross-codec calls is a codec tag OR-ed with that codec's order word
CODEC_RANS4X16 = 0
CODEC_ARITH = 1 << 24
CODEC_MASK = 0x0F000000
# part 2n: a fqzcomp_qual strategy among the methods of the quality calls
CODEC_FQZ = 3 << 24

_tls = threading.local()


def _thread_ctx():
    """One context per host thread, kept between calls: it owns the device arenas, the pinned bounce buffers
    and the lane contexts of the host-batch pipeline, which are far too expensive to rebuild per call."""
    ctx = getattr(_tls, "ctx", None)
    if ctx is None:
        ctx = _tls.ctx = _Ctx()
    return ctx


def set_option(name, value):
    """rans4x16_hip_set_option on the calling thread's context (the one the host-batch helpers below use)."""
    _thread_ctx().set_option(name, value)


def get_option(name):
    return _thread_ctx().get_option(name)


def route_read(which, reset=True):
    """The route read-out of the calling thread's context (the one the host-batch helpers use): see _Ctx.route_read."""
    return _thread_ctx().route_read(which, reset)


def get_default_option(name):
    v = C.c_long(0)
    if _lib.load().rans4x16_hip_get_option(None, name.encode(), C.byref(v)) != 0:
        raise KeyError(f"unknown option {name!r}")
    return v.value


def set_default_option(name, value):
    """Process-wide default (ctx == NULL): contexts created from now on, and the combiner if it has not started."""
    if _lib.load().rans4x16_hip_set_option(None, name.encode(), int(value)) != 0:
        raise KeyError(f"unknown option {name!r}")


def _host_batch(blocks, decode, orders=None, caps=None):
    ctx = _thread_ctx()
    L = ctx.L
    a = _HostArrays(blocks, caps if decode else lambda i, size: L.rans_compress_bound_4x16(size, orders[i]))
    if decode:
        rc = L.rans4x16_hip_uncompress_batch(ctx.h, a.n, a.in_p, a.in_sz, a.out_p, a.out_sz, a.status)
    else:
        rc = L.rans4x16_hip_compress_batch(ctx.h, a.n, a.in_p, a.in_sz, a.out_p, a.out_sz, _methods(orders), a.status)
    if rc < 0:
        raise RuntimeError("batch call failed: " + ctx.error())
    return a.results()


class MultiCodec:
    """Host-buffer batches over several GPUs of one node (include/rans4x16_hip.h part 3): the library cuts the
    batch into contiguous ranges, one per device.  devices=None: every visible device; a device may be listed
    twice (two pipelines on one card)."""

    def __init__(self, devices=None):
        self.L = _lib.load()
        if devices is None:
            self.h = self.L.rans4x16_hip_multi_create(0, None)
        else:
            arr = (C.c_int * len(devices))(*devices)
            self.h = self.L.rans4x16_hip_multi_create(len(devices), arr)
        if not self.h:
            raise RuntimeError("rans4x16_hip_multi_create failed: no usable HIP device (no CPU path exists)")

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.rans4x16_hip_multi_destroy(self.h)
        except Exception:
            pass

    def devices(self):
        return self.L.rans4x16_hip_multi_devices(self.h)

    def _run(self, blocks, decode, orders=None, caps=None):
        L = self.L
        a = _HostArrays(blocks, caps if decode else lambda i, size: L.rans_compress_bound_4x16(size, orders[i]))
        if decode:
            rc = L.rans4x16_hip_uncompress_batch_multi(self.h, a.n, a.in_p, a.in_sz, a.out_p, a.out_sz, a.status)
        else:
            rc = L.rans4x16_hip_compress_batch_multi(self.h, a.n, a.in_p, a.in_sz, a.out_p, a.out_sz, _methods(orders), a.status)
        if rc < 0:
            raise RuntimeError("multi-device batch failed: " + L.rans4x16_hip_multi_last_error(self.h).decode())
        return a.results()

    def compress_batch(self, blocks, orders):
        return self._run(blocks, False, orders=orders)

    def uncompress_batch(self, blocks, caps):
        return self._run(blocks, True, caps=caps)


def compress_batch(blocks, orders):
    """list of bytes, list of int -> (list of bytes|None, list of status)."""
    return _host_batch(blocks, False, orders=orders)


def compress_best_batch(blocks, methods):
    """The reference's caller-side "try several methods, keep the smallest" loop (tokenise_name3.c:1246-1300)
    as one call: list of bytes, list of order values -> (list of bytes|None, chosen order per block, statuses)."""
    ctx = _thread_ctx()
    L = ctx.L
    a = _HostArrays(blocks, lambda i, size: max(L.rans_compress_bound_4x16(size, m) for m in methods))
    chosen = (C.c_int * a.n)()
    rc = L.rans4x16_hip_compress_best_batch(ctx.h, a.n, a.in_p, a.in_sz, a.out_p, a.out_sz, len(methods), _methods(methods), chosen, a.status)
    if rc < 0:
        raise RuntimeError("batch call failed: " + ctx.error())
    res, status = a.results()
    return res, list(chosen), status


def uncompress_batch(blocks, caps):
    """list of compressed bytes, list of output capacities -> (list of bytes|None, statuses)."""
    return _host_batch(blocks, True, caps=caps)


def tok3_scan(container, max_columns=0, max_col_size=0):
    """rans4x16_hip_tok3_scan: walk one tok3 column container (bytes) on the host.  Returns (status, info): status 0 or the
    R4X16_E_* code the device walk gives, info a dict with last_start, nreads, ndesc, ncol, total_col_size, largest_col
    and largest_stream (after a failure: of the columns accepted before it).  Needs no GPU."""
    L = _lib.load()
    buf = bytes(container)
    u32 = [C.c_uint32(0) for _ in range(6)]
    total = C.c_uint64(0)
    rc = L.rans4x16_hip_tok3_scan(buf, len(buf), int(max_columns), int(max_col_size), C.byref(u32[0]), C.byref(u32[1]),
                                  C.byref(u32[2]), C.byref(u32[3]), C.byref(total), C.byref(u32[4]), C.byref(u32[5]))
    if rc < 0:
        raise ValueError("tok3_scan: bad arguments")
    return rc, {"last_start": u32[0].value, "nreads": u32[1].value, "ndesc": u32[2].value, "ncol": u32[3].value,
                "total_col_size": total.value, "largest_col": u32[4].value, "largest_stream": u32[5].value}


def tok3_scan_any(container, max_columns=0, max_col_size=0):
    """rans4x16_hip_tok3_scan_any: tok3_scan for either flavour.  Returns (status, info, use_arith): a container whose byte
    8 is set is walked by the same rules, not refused, and use_arith is 1 for it.  Needs no GPU."""
    L = _lib.load()
    buf = bytes(container)
    u32 = [C.c_uint32(0) for _ in range(6)]
    total = C.c_uint64(0)
    arith = C.c_int(0)
    rc = L.rans4x16_hip_tok3_scan_any(buf, len(buf), int(max_columns), int(max_col_size), C.byref(u32[0]), C.byref(u32[1]),
                                      C.byref(u32[2]), C.byref(u32[3]), C.byref(total), C.byref(u32[4]), C.byref(u32[5]),
                                      C.byref(arith))
    if rc < 0:
        raise ValueError("tok3_scan_any: bad arguments")
    return rc, {"last_start": u32[0].value, "nreads": u32[1].value, "ndesc": u32[2].value, "ncol": u32[3].value,
                "total_col_size": total.value, "largest_col": u32[4].value, "largest_stream": u32[5].value}, arith.value


TOK3_ARITH_DECODE, TOK3_ARITH_ENCODE = 1, 2


def set_tok3_arith(mode, ctx=None):
    """rans4x16_hip_set_tok3_arith on the calling thread's context (or `ctx`): returns the previous mode."""
    ctx = ctx or _thread_ctx()
    was = ctx.L.rans4x16_hip_set_tok3_arith(ctx.h, int(mode))
    if was < 0:
        raise ValueError("set_tok3_arith: %r is outside 0..3" % (mode,))
    return was


def thread_tok3_arith(mode):
    """rans4x16_hip_set_tok3_arith on rans4x16_hip_thread_ctx(), the library's own context of the calling thread - the one
    the single-block symbols (encode_names, decode_names, ..) run on: returns the previous mode.  Needs a GPU."""
    L = _lib.load()
    h = L.rans4x16_hip_thread_ctx()
    if not h:
        raise RuntimeError("rans4x16_hip_thread_ctx: no usable HIP device")
    was = L.rans4x16_hip_set_tok3_arith(h, int(mode))
    if was < 0:
        raise ValueError("set_tok3_arith: %r is outside 0..3" % (mode,))
    return was


def tok3_level_methods(level):
    """rans4x16_hip_tok3_level_methods: the method list encode_names tries per column at `level`.  Needs no GPU."""
    m = (C.c_int * 9)()
    k = _lib.load().rans4x16_hip_tok3_level_methods(int(level), m)
    return list(m[:k])


def _methods(methods):
    """A list of order values as a C int array: the methods of a best-of-k call, the orders of a host batch."""
    return (C.c_int * len(methods))(*[int(m) for m in methods])


def _free(addr):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free.restype = None
    libc.free(addr)


def set_names_chunk_blocks(blocks, ctx=None):
    """rans4x16_hip_set_names_chunk_blocks on the calling thread's context: at most `blocks` blocks per chunk of the
    names batches below (0: by room alone)."""
    ctx = ctx or _thread_ctx()
    if ctx.L.rans4x16_hip_set_names_chunk_blocks(ctx.h, int(blocks)) != 0:
        raise ValueError("names_chunk_blocks: %r" % (blocks,))


def _names_batch(blocks, encode, methods=None, ctx=None, tok3_arith=None):
    """Either names batch with out[i] == NULL: the library allocates exactly the results.  tok3_arith: None leaves the
    context's mode alone; 0 / 1 runs the call without / with the arith flavour and puts the context's mode back."""
    ctx = ctx or _thread_ctx()
    if tok3_arith is not None:
        was = set_tok3_arith((TOK3_ARITH_ENCODE if encode else TOK3_ARITH_DECODE) if tok3_arith else 0, ctx)
        try:
            return _names_batch(blocks, encode, methods, ctx)
        finally:
            set_tok3_arith(was, ctx)
    L = ctx.L
    n = len(blocks)
    srcs = [np.frombuffer(bytes(b), dtype=np.uint8) for b in blocks]
    dummy = np.zeros(1, dtype=np.uint8)
    in_p = (C.c_void_p * n)(*[(s.ctypes.data if len(s) else dummy.ctypes.data) for s in srcs])
    in_sz = (C.c_uint * n)(*[len(s) for s in srcs])
    out_p = (C.c_void_p * n)()
    out_sz = (C.c_uint * n)()
    a, b = (C.c_uint * n)(), (C.c_uint * n)()
    status = (C.c_int * n)()
    if encode:
        meth = _methods(methods)
        rc = L.rans4x16_hip_tok3_encode_names_batch(ctx.h, n, in_p, in_sz, out_p, out_sz, len(methods), meth, a, b, status)
    else:
        rc = L.rans4x16_hip_tok3_decode_names_batch(ctx.h, n, in_p, in_sz, out_p, out_sz, a, status)
    res = []
    for i in range(n):
        res.append(C.string_at(out_p[i], out_sz[i]) if out_p[i] and status[i] == 0 and rc >= 0 else None)
        if out_p[i]:
            _free(out_p[i])
    if rc < 0:
        raise RuntimeError("names batch failed: " + ctx.error())
    return res, list(a), list(b), list(status)


def tok3_encode_names_batch(blocks, level=None, methods=None, ctx=None, tok3_arith=None):
    """encode_names over a list of name blocks (bytes) in one call: (containers | None, last_starts, statuses).  The method
    list is `methods`, or that of `level` (tok3_level_methods); nreads of block i is in container i's header.  tok3_arith:
    1 writes the arith flavour (use_arith = 1), 0 the rANS one, None what the context's mode says (set_tok3_arith)."""
    if methods is None:
        methods = tok3_level_methods(9 if level is None else level)
    res, last_start, _, status = _names_batch(blocks, True, methods=list(methods), ctx=ctx, tok3_arith=tok3_arith)
    return res, last_start, status


def tok3_decode_names_batch(containers, ctx=None, tok3_arith=None):
    """decode_names over a list of containers in one call: (names | None - NUL-separated, last_start bytes -, statuses).
    tok3_arith: 1 reads either flavour, block by block; 0 the rANS one alone; None what the context's mode says."""
    res, _, _, status = _names_batch(containers, False, ctx=ctx, tok3_arith=tok3_arith)
    return res, status


def encode_names(block, level, use_arith=0):
    """The single-block drop-in symbol: bytes -> (container, last_start) or None.  The caller's buffer is a copy here, so
    the NULs the call writes over the separators are not seen.  use_arith != 0 goes to the arith flavour's symbol, as
    include/tok3_names_hip.h forwards it."""
    L = _lib.load()
    buf = C.create_string_buffer(bytes(block), max(len(block), 1))
    out_len, last_start = C.c_int(0), C.c_int(0)
    if use_arith:
        p = L.rans4x16_hip_tok3_arith_encode_names(buf, len(block), int(level), C.byref(out_len), C.byref(last_start))
    else:
        p = L.rans4x16_hip_tok3_encode_names(buf, len(block), int(level), 0, C.byref(out_len), C.byref(last_start))
    if not p:
        return None
    res = C.string_at(p, out_len.value)
    _free(p)
    return res, last_start.value


def decode_names(container):
    """The single-block drop-in symbol: container bytes -> NUL-separated names or None.  A container whose byte 8
    (use_arith) is set goes to the arith flavour's symbol, as include/tok3_names_hip.h forwards it."""
    L = _lib.load()
    buf = bytes(container)
    out_len = C.c_uint32(0)
    fn = L.rans4x16_hip_tok3_arith_decode_names if len(buf) > 8 and buf[8] else L.rans4x16_hip_tok3_decode_names
    p = fn(buf, len(buf), C.byref(out_len))
    if not p:
        return None
    res = C.string_at(p, out_len.value)
    _free(p)
    return res


def arith_uncompress_batch(blocks, caps, ctx=None):
    """rans4x16_hip_arith_uncompress_batch: arith_dynamic streams (bytes) and the capacity of each output ->
    (list of bytes | None, statuses).  One upload, one device call, one download."""
    ctx = ctx or _thread_ctx()
    a = _HostArrays(blocks, caps)
    rc = ctx.L.rans4x16_hip_arith_uncompress_batch(ctx.h, a.n, a.in_p, a.in_sz, a.out_p, a.out_sz, a.status)
    if rc < 0:
        raise RuntimeError("arith batch failed: " + ctx.error())
    return a.results()


def arith_uncompress(comp, out_size=None):
    """The reference's arith_uncompress (out_size None) / arith_uncompress_to with a buffer of out_size bytes: the decoded
    bytes, or None where the reference returns NULL."""
    L = _lib.load()
    buf = bytes(comp)
    n = C.c_uint(0 if out_size is None else int(out_size))
    if out_size is None:
        p = L.rans4x16_hip_arith_uncompress(buf, len(buf), C.byref(n))
        if not p:
            return None
        res = C.string_at(p, n.value)
        _free(p)
        return res
    out = C.create_string_buffer(max(int(out_size), 1))
    p = L.rans4x16_hip_arith_uncompress_to(buf, len(buf), out, C.byref(n))
    return out.raw[:n.value] if p else None


def fqz_scan(stream):
    """rans4x16_hip_fqz_scan: the header walk of one fqzcomp_qual stream.  Returns (status, info) with info the stored size,
    the header's bytes, gflags, nparam, max_sel and max_sym.  Needs no GPU."""
    L = _lib.load()
    buf = bytes(stream)
    v = [C.c_uint32(0) for _ in range(6)]
    st = L.rans4x16_hip_fqz_scan(buf, len(buf), *[C.byref(x) for x in v])
    keys = ("stored_size", "header_bytes", "gflags", "nparam", "max_sel", "max_sym")
    return st, dict(zip(keys, (x.value for x in v)))


def fqz_uncompress_batch(blocks, caps=None, nlengths=None, ctx=None):
    """rans4x16_hip_fqz_uncompress_batch: fqzcomp_qual streams (bytes) -> (list of bytes | None, statuses, lengths, nrec).
    caps: the capacity of each output (default: the stored size); nlengths: how many record lengths to take per block
    (default: none) - lengths[i] holds min(nlengths[i], nrec[i]) entries.  One upload, one device call, one download."""
    ctx = ctx or _thread_ctx()
    L = ctx.L
    n = len(blocks)
    if caps is None:
        caps = [fqz_scan(b)[1]["stored_size"] for b in blocks]
    a = _HostArrays(blocks, caps)
    nl = [0] * n if nlengths is None else [int(v) for v in nlengths]
    lens = [np.full(max(v, 1), -1, dtype=np.int32) for v in nl]
    len_p = (C.c_void_p * n)(*[x.ctypes.data for x in lens])
    nl_a = (C.c_int * n)(*nl)
    nrec = (C.c_uint * n)()
    rc = L.rans4x16_hip_fqz_uncompress_batch(ctx.h, n, a.in_p, a.in_sz, a.out_p, a.out_sz, a.status, len_p, nl_a, nrec)
    if rc < 0:
        raise RuntimeError("fqz batch failed: " + ctx.error())
    res, status = a.results()
    return res, status, [lens[i][:min(nl[i], nrec[i])].tolist() for i in range(n)], list(nrec)


def fqz_decompress(comp, nlengths=0):
    """The reference's fqz_decompress: (the decoded qualities, the first nlengths record lengths - the entries behind the
    last record are -1), or None where the reference returns NULL."""
    L = _lib.load()
    buf = bytes(comp)
    n = C.c_size_t(0)
    lens = (C.c_int * max(int(nlengths), 1))(*([-1] * max(int(nlengths), 1)))
    p = L.rans4x16_hip_fqz_decompress(buf, len(buf), C.byref(n), lens if nlengths else None, int(nlengths))
    if not p:
        return None
    res = C.string_at(p, n.value)
    _free(p)
    return res, list(lens)[:int(nlengths)]


def fqz_pick_parameters(data, lens, flags, vers=4, strat=0, params_cap=None):
    """rans4x16_hip_fqz_pick_parameters: the reference's parameter choice for one slice.  Returns (status, the parameter
    bytes or None, lens, flags) - the lists as the call leaves them: the lengths after the reference's fix-ups, the selector
    in flags[rec] >> 16.  params_cap: the room offered (default: enough); status 1 gives (1, the size needed, ..).  Needs no
    GPU."""
    L = _lib.load()
    buf = bytes(data)
    n = len(lens)
    la = (C.c_uint32 * max(n, 1))(*[int(v) & 0xffffffff for v in lens])
    fa = (C.c_uint32 * max(n, 1))(*[int(v) & 0xffffffff for v in flags])
    cap = 4096 if params_cap is None else int(params_cap)
    out = C.create_string_buffer(max(cap, 1))
    size = C.c_uint(0)
    st = L.rans4x16_hip_fqz_pick_parameters(int(vers), int(strat), n, la, fa, buf, len(buf), out, cap, C.byref(size))
    if st == 1 and params_cap is None:
        cap = size.value
        out = C.create_string_buffer(max(cap, 1))
        st = L.rans4x16_hip_fqz_pick_parameters(int(vers), int(strat), n, la, fa, buf, len(buf), out, cap, C.byref(size))
    res = out.raw[:size.value] if st == 0 else (size.value if st == 1 else None)
    return st, res, list(la)[:n], list(fa)[:n]


def fqz_compress_cap(size, nrec, params_size):
    """rans4x16_hip_fqz_compress_cap: a capacity with which a block of `size` bytes in `nrec` records never overflows."""
    return _lib.load().rans4x16_hip_fqz_compress_cap(int(size), int(nrec), int(params_size))


def fqz_pick_cap():
    """rans4x16_hip_fqz_pick_cap: a parameter slot of this many bytes holds whatever the device pick writes."""
    return _lib.load().rans4x16_hip_fqz_pick_cap()


def fqz_compress_batch(blocks, lens, flags, vers=4, strat=0, params=None, caps=None, ctx=None):
    """rans4x16_hip_fqz_compress_batch: quality blocks (bytes) with their record lengths and flags -> (list of bytes | None,
    statuses, lens, flags as the call leaves them).  params: None, or per block None (picked on the host with vers and
    strat) or its parameter bytes.  caps: the capacity of each output (default: fqz_compress_cap with 4096 parameter
    bytes).  One upload, one device call, one download."""
    ctx = ctx or _thread_ctx()
    L = ctx.L
    n = len(blocks)
    la = [np.array([int(v) & 0xffffffff for v in x], dtype=np.uint32) for x in lens]
    fa = [np.array([int(v) & 0xffffffff for v in x], dtype=np.uint32) for x in flags]
    pars = [None if params is None or p is None else np.frombuffer(bytes(p), dtype=np.uint8) for p in (params or [None] * n)]
    if caps is None:
        caps = lambda i, size: L.rans4x16_hip_fqz_compress_cap(size, len(la[i]), 4096 if pars[i] is None else len(pars[i]))
    a = _HostArrays(blocks, caps)
    dummy = np.zeros(4, dtype=np.uint8)
    ptr = lambda x: x.ctypes.data if len(x) else dummy.ctypes.data
    len_p = (C.c_void_p * n)(*[ptr(x) for x in la])
    fl_p = (C.c_void_p * n)(*[ptr(x) for x in fa])
    par_p = (C.c_void_p * n)(*[None if p is None else ptr(p) for p in pars])
    nrec = (C.c_uint * n)(*[len(x) for x in la])
    par_sz = (C.c_uint * n)(*[0 if p is None else len(p) for p in pars])
    rc = L.rans4x16_hip_fqz_compress_batch(ctx.h, n, a.in_p, a.in_sz, nrec, len_p, fl_p, int(vers), int(strat),
                                           None if params is None else par_p, par_sz, a.out_p, a.out_sz, a.status)
    if rc < 0:
        raise RuntimeError("fqz batch failed: " + ctx.error())
    res, status = a.results()
    return res, status, [x.tolist() for x in la], [x.tolist() for x in fa]


def fqz_compress_best_batch(blocks, lens, flags, strats, vers=4, caps=None, ctx=None):
    """rans4x16_hip_fqz_compress_best_batch: quality blocks (bytes) with their record lengths and flags, each coded under
    every strategy of `strats` and the smallest stream kept -> (list of bytes | None, statuses, the winners' indices into
    strats (-1: none), lens, flags as the call leaves them).  caps: the capacity of each output (default: fqz_compress_cap
    with fqz_pick_cap parameter bytes).  One upload, one device call, one download."""
    ctx = ctx or _thread_ctx()
    L = ctx.L
    n = len(blocks)
    la = [np.array([int(v) & 0xffffffff for v in x], dtype=np.uint32) for x in lens]
    fa = [np.array([int(v) & 0xffffffff for v in x], dtype=np.uint32) for x in flags]
    if caps is None:
        caps = lambda i, size: L.rans4x16_hip_fqz_compress_cap(size, len(la[i]), L.rans4x16_hip_fqz_pick_cap())
    a = _HostArrays(blocks, caps)
    dummy = np.zeros(4, dtype=np.uint8)
    ptr = lambda x: x.ctypes.data if len(x) else dummy.ctypes.data
    len_p = (C.c_void_p * n)(*[ptr(x) for x in la])
    fl_p = (C.c_void_p * n)(*[ptr(x) for x in fa])
    nrec = (C.c_uint * n)(*[len(x) for x in la])
    chosen = (C.c_int * n)(*([-1] * n))
    st = (C.c_int * len(strats))(*[int(v) for v in strats])
    rc = L.rans4x16_hip_fqz_compress_best_batch(ctx.h, n, a.in_p, a.in_sz, nrec, len_p, fl_p, int(vers), len(strats), st,
                                                a.out_p, a.out_sz, chosen, a.status)
    if rc < 0:
        raise RuntimeError("fqz best batch failed: " + ctx.error())
    res, status = a.results()
    return res, status, list(chosen), [x.tolist() for x in la], [x.tolist() for x in fa]


class _FqzSlice(C.Structure):
    _fields_ = [("num_records", C.c_int), ("len", C.POINTER(C.c_uint32)), ("flags", C.POINTER(C.c_uint32))]


def fqz_compress(data, lens, flags, vers=4, strat=0, gp=None):
    """The reference's fqz_compress(vers, slice, in, in_size, &out_size, strat, gp): (the stream, lens, flags as the call
    leaves them), or None where it returns NULL (gp must be None: the parameter struct is not taken)."""
    L = _lib.load()
    buf = C.create_string_buffer(bytes(data), max(len(data), 1))
    n = len(lens)
    la = (C.c_uint32 * max(n, 1))(*[int(v) & 0xffffffff for v in lens])
    fa = (C.c_uint32 * max(n, 1))(*[int(v) & 0xffffffff for v in flags])
    s = _FqzSlice(n, la, fa)
    size = C.c_size_t(0)
    p = L.rans4x16_hip_fqz_compress(int(vers), C.byref(s), buf, len(data), C.byref(size), int(strat), gp)
    if buf.raw[:len(data)] != bytes(data):
        raise AssertionError("fqz_compress changed its input")
    if not p:
        return None
    res = C.string_at(p, size.value)
    _free(p)
    return res, list(la)[:n], list(fa)[:n]


def arith_compress_bound(size, order):
    """The reference's arith_compress_bound (host arithmetic)."""
    return _lib.load().rans4x16_hip_arith_compress_bound(int(size), int(order))


def arith_compress_cap(size, order):
    """rans4x16_hip_arith_compress_cap: the smallest capacity a block of `size` bytes is accepted with under `order`."""
    return _lib.load().rans4x16_hip_arith_compress_cap(int(size), int(order))


def arith_compress_batch(blocks, orders, caps=None, ctx=None):
    """rans4x16_hip_arith_compress_batch: blocks (bytes) and the order word of each -> (list of bytes | None, statuses).
    caps: the capacity of each output (default: arith_compress_cap).  One upload, one device call, one download."""
    ctx = ctx or _thread_ctx()
    L = ctx.L
    if caps is None:
        caps = [L.rans4x16_hip_arith_compress_cap(len(b), int(o)) for b, o in zip(blocks, orders)]
    a = _HostArrays(blocks, caps)
    rc = L.rans4x16_hip_arith_compress_batch(ctx.h, a.n, a.in_p, a.in_sz, a.out_p, a.out_sz, _methods(orders), a.status)
    if rc < 0:
        raise RuntimeError("arith batch failed: " + ctx.error())
    return a.results()


def arith_compress(data, order, out_size=None):
    """The reference's arith_compress (out_size None) / arith_compress_to with a buffer of out_size bytes: the stream, or
    None where the call returns NULL."""
    L = _lib.load()
    buf = bytes(data)
    n = C.c_uint(0 if out_size is None else int(out_size))
    if out_size is None:
        p = L.rans4x16_hip_arith_compress(buf, len(buf), C.byref(n), int(order))
        if not p:
            return None
        res = C.string_at(p, n.value)
        _free(p)
        return res
    out = C.create_string_buffer(max(int(out_size), 1))
    p = L.rans4x16_hip_arith_compress_to(buf, len(buf), out, C.byref(n), int(order))
    return out.raw[:n.value] if p else None


def compress_best_any_batch(blocks, methods, caps=None, ctx=None):
    """rans4x16_hip_compress_best_any_batch: every block under a list of tagged methods (CODEC_ARITH | order for
    arith_dynamic, a plain order word for rANS 4x16), the smallest stream kept.  caps None: the library allocates exactly
    the result; else a capacity per block.  Returns (the streams, None for a block that failed; the chosen methods; the
    statuses)."""
    ctx = ctx or _thread_ctx()
    L = ctx.L
    n = len(blocks)
    meth = _methods(methods)
    chosen = (C.c_int * n)()
    if caps is None:
        call = lambda n, in_p, in_sz, out_p, out_sz, status: L.rans4x16_hip_compress_best_any_batch(
            ctx.h, n, in_p, in_sz, out_p, out_sz, len(methods), meth, chosen, status)
        outs, status = _library_allocates(blocks, call, "compress_best_any_batch", ctx)
        return outs, list(chosen), status
    a = _HostArrays(blocks, caps)
    rc = L.rans4x16_hip_compress_best_any_batch(ctx.h, n, a.in_p, a.in_sz, a.out_p, a.out_sz, len(methods), meth, chosen, a.status)
    if rc < 0:
        raise RuntimeError("compress_best_any_batch: " + ctx.error())
    outs, status = a.results()
    return outs, list(chosen), status


def uncompress_any_batch(blocks, methods, caps, ctx=None):
    """rans4x16_hip_uncompress_any_batch: streams of either codec, methods[i] saying which (only its codec tag is looked
    at; negative: a block that was never written), into buffers of caps[i] bytes.  Returns (the blocks, None where one
    failed; the statuses)."""
    ctx = ctx or _thread_ctx()
    a = _HostArrays(blocks, caps)
    rc = ctx.L.rans4x16_hip_uncompress_any_batch(ctx.h, a.n, a.in_p, a.in_sz, _methods(methods), a.out_p, a.out_sz, a.status)
    if rc < 0:
        raise RuntimeError("uncompress_any_batch: " + ctx.error())
    return a.results()


def compress_best_qual_batch(blocks, lens, flags, methods, vers=4, caps=None, ctx=None):
    """rans4x16_hip_compress_best_qual_batch: quality blocks (bytes) with their record lengths and flags under a list of
    tagged methods (a plain order word for rANS 4x16, CODEC_ARITH | order, CODEC_FQZ | strat), the smallest stream kept.
    caps None: the library allocates exactly the result; else a capacity per block.  Returns (the streams, None for a block
    that failed; the chosen methods; the statuses; lens and flags as the call leaves them - changed only where
    fqzcomp_qual won)."""
    ctx = ctx or _thread_ctx()
    L = ctx.L
    n = len(blocks)
    meth = _methods(methods)
    la = [np.array([int(v) & 0xffffffff for v in x], dtype=np.uint32) for x in lens]
    fa = [np.array([int(v) & 0xffffffff for v in x], dtype=np.uint32) for x in flags]
    dummy = np.zeros(4, dtype=np.uint8)
    ptr = lambda x: x.ctypes.data if len(x) else dummy.ctypes.data
    len_p = (C.c_void_p * n)(*[ptr(x) for x in la])
    fl_p = (C.c_void_p * n)(*[ptr(x) for x in fa])
    nrec = (C.c_uint * n)(*[len(x) for x in la])
    chosen = (C.c_int * n)(*([-1] * n))
    back = lambda: ([x.tolist() for x in la], [x.tolist() for x in fa])
    if caps is None:
        call = lambda n, in_p, in_sz, out_p, out_sz, status: L.rans4x16_hip_compress_best_qual_batch(
            ctx.h, n, in_p, in_sz, nrec, len_p, fl_p, int(vers), out_p, out_sz, len(methods), meth, chosen, status)
        outs, status = _library_allocates(blocks, call, "compress_best_qual_batch", ctx)
        return (outs, list(chosen), status) + back()
    a = _HostArrays(blocks, caps)
    rc = L.rans4x16_hip_compress_best_qual_batch(ctx.h, n, a.in_p, a.in_sz, nrec, len_p, fl_p, int(vers), a.out_p, a.out_sz, len(methods), meth,
                                                 chosen, a.status)
    if rc < 0:
        raise RuntimeError("compress_best_qual_batch: " + ctx.error())
    outs, status = a.results()
    return (outs, list(chosen), status) + back()


def uncompress_qual_batch(blocks, methods, caps, nlengths=None, ctx=None):
    """rans4x16_hip_uncompress_qual_batch: streams of the three codecs, methods[i] saying which (only its codec tag is looked
    at; negative: a block that was never written), into buffers of caps[i] bytes.  nlengths: how many record lengths to take
    per block (default: none).  Returns (the blocks, None where one failed; the statuses; the lengths - min(nlengths[i],
    nrec[i]) entries for a CODEC_FQZ block; nrec, 0 for the other codecs' blocks)."""
    ctx = ctx or _thread_ctx()
    a = _HostArrays(blocks, caps)
    n = a.n
    nl = [0] * n if nlengths is None else [int(v) for v in nlengths]
    lens = [np.full(max(v, 1), -1, dtype=np.int32) for v in nl]
    len_p = (C.c_void_p * n)(*[x.ctypes.data for x in lens])
    nl_a = (C.c_int * n)(*nl)
    nrec = (C.c_uint * n)()
    rc = ctx.L.rans4x16_hip_uncompress_qual_batch(ctx.h, n, a.in_p, a.in_sz, _methods(methods), a.out_p, a.out_sz, a.status, len_p, nl_a, nrec)
    if rc < 0:
        raise RuntimeError("uncompress_qual_batch: " + ctx.error())
    res, status = a.results()
    return res, status, [lens[i][:min(nl[i], nrec[i])].tolist() for i in range(n)], list(nrec)


class DeviceCodec:
    """Device-resident batches on torch tensors (torch is used for device memory and streams
    only).  All tensors must live on the context's device."""

    def __init__(self, device_index=0):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", device_index)
        with torch.cuda.device(self.dev):
            self.ctx = _Ctx(device_index)
        self.L = self.ctx.L

    def timing(self, enable=True):
        self.L.rans4x16_hip_timing(self.ctx.h, 1 if enable else 0)

    def set_option(self, name, value):
        self.ctx.set_option(name, value)

    def get_option(self, name):
        return self.ctx.get_option(name)

    def route_read(self, which, reset=True):
        return self.ctx.route_read(which, reset)

    def timing_read(self, which, reset=True):
        ms = C.c_double(0)
        k = C.c_int(0)
        rc = self.L.rans4x16_hip_timing_read(self.ctx.h, which, C.byref(ms), C.byref(k), 1 if reset else 0)
        if rc != 0:
            raise RuntimeError("timing_read failed")
        return ms.value, k.value

    def workspace_bytes(self):
        return self.L.rans4x16_hip_workspace_bytes(self.ctx.h)

    def residency(self, decode, nsym, order, shift=10, kind=0):
        """(streams per CU, live lanes per wave, CUs) of the chain kernel for this kind of stream.  kind: 0 the full
        chip's rows, R4X16_RES_SHORT (2) the short-step kind, R4X16_RES_MID (4) the mid rows (include/rans4x16_hip.h)."""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        if self.L.rans4x16_hip_residency(self.ctx.h, (1 if decode else 0) | int(kind), nsym, order, shift,
                                         C.byref(a), C.byref(b), C.byref(c)) != 0:
            raise RuntimeError("residency query failed")
        return a.value, b.value, c.value

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def compress(self, d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status, order,
                 max_in_size, d_order=None, total_in_size=0):
        self._slot_args(d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status)
        n = in_off.numel()
        rc = self.L.rans4x16_hip_compress_dev_sized(
            self.ctx.h, n, d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(), out_size.data_ptr(),
            status.data_ptr(), int(order), d_order.data_ptr() if d_order is not None else None,
            int(max_in_size), int(total_in_size), self._stream())
        self._check(rc, "compress_dev")

    def set_stripe_encode(self, max_planes):
        """rans4x16_hip_set_dev_stripe_encode: `compress` with d_order encodes X_STRIPE blocks of up to max_planes
        planes (0: off, such blocks report UNSUPPORTED)."""
        if self.L.rans4x16_hip_set_dev_stripe_encode(self.ctx.h, int(max_planes)) != 0:
            raise ValueError(f"set_stripe_encode: {max_planes!r} is outside 0..255")

    def compress_best(self, d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status, methods,
                      max_in_size, chosen=None, total_in_size=0):
        """rans4x16_hip_compress_best_dev: every block with each of `methods` (a list of order values), the smallest
        result in its output slot, the winning method in `chosen` (int32 tensor, optional).  Enqueues only."""
        t = self.torch
        self._slot_args(d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status)
        assert chosen is None or chosen.dtype == t.int32
        n = in_off.numel()
        meth = _methods(methods)
        rc = self.L.rans4x16_hip_compress_best_dev(
            self.ctx.h, n, d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(), out_size.data_ptr(),
            status.data_ptr(), len(methods), meth, chosen.data_ptr() if chosen is not None else None,
            int(max_in_size), int(total_in_size), self._stream())
        self._check(rc, "compress_best_dev")

    def uncompress(self, d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status,
                   max_in_size, max_out_cap, total_out_cap=0):
        self._slot_args(d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status)
        n = in_off.numel()
        rc = self.L.rans4x16_hip_uncompress_dev_sized(
            self.ctx.h, n, d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(), out_size.data_ptr(),
            status.data_ptr(), int(max_in_size), int(max_out_cap), int(total_out_cap), self._stream())
        self._check(rc, "uncompress_dev")

    # ---- arith_dynamic, both directions (include/rans4x16_hip.h parts 2g, 2h) --------------------------------------------------
    def arith_uncompress(self, d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status,
                         max_in_size, max_out_size, total_out_size=0):
        """rans4x16_hip_arith_uncompress_dev: uncompress()'s arguments over arith_dynamic streams.  Enqueues only."""
        self._slot_args(d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status)
        rc = self.L.rans4x16_hip_arith_uncompress_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(), out_size.data_ptr(),
            status.data_ptr(), int(max_in_size), int(max_out_size), int(total_out_size), self._stream())
        self._check(rc, "arith_uncompress_dev")

    def arith_compress(self, d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status, order,
                       max_in_size, d_order=None, total_in_size=0):
        """rans4x16_hip_arith_compress_dev: compress()'s arguments, arith_dynamic streams out.  Enqueues only.  X_STRIPE
        under d_order needs set_stripe_encode."""
        t = self.torch
        self._slot_args(d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status)
        assert d_order is None or d_order.dtype == t.int32
        rc = self.L.rans4x16_hip_arith_compress_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(), out_size.data_ptr(),
            status.data_ptr(), int(order), d_order.data_ptr() if d_order is not None else None,
            int(max_in_size), int(total_in_size), self._stream())
        self._check(rc, "arith_compress_dev")

    def arith_peek(self, d_in, in_off, in_size, fmt, raw_size, status, max_in_size):
        """rans4x16_hip_arith_peek_dev: peek()'s arguments and results over arith_dynamic streams."""
        t = self.torch
        assert d_in.dtype == t.uint8 and in_off.dtype == t.int64 and in_size.dtype == t.int32
        assert fmt.dtype == t.int32 and raw_size.dtype == t.int32 and status.dtype == t.int32
        rc = self.L.rans4x16_hip_arith_peek_dev(self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
                                                fmt.data_ptr(), raw_size.data_ptr(), status.data_ptr(), int(max_in_size), self._stream())
        self._check(rc, "arith_peek_dev")

    # ---- fqzcomp_qual decoding (include/rans4x16_hip.h part 2i) -------------------------------------------------------
    def fqz_uncompress(self, d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status,
                       max_in_size, max_out_size, total_out_size=0, d_len=None, len_off=None, len_cap=None, nrec=None):
        """rans4x16_hip_fqz_uncompress_dev: arith_uncompress()'s arguments over fqzcomp_qual streams, and the four optional
        ones: record lengths into d_len (int32) at len_off (int64, entries) up to len_cap (int32, entries), record counts
        into nrec (int32).  Enqueues only."""
        t = self.torch
        self._slot_args(d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status)
        assert d_len is None or (d_len.dtype == t.int32 and len_off.dtype == t.int64 and len_cap.dtype == t.int32)
        assert nrec is None or nrec.dtype == t.int32
        ptr = lambda x: x.data_ptr() if x is not None else None
        rc = self.L.rans4x16_hip_fqz_uncompress_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(), out_size.data_ptr(), status.data_ptr(),
            ptr(d_len), ptr(len_off), ptr(len_cap), ptr(nrec),
            int(max_in_size), int(max_out_size), int(total_out_size), self._stream())
        self._check(rc, "fqz_uncompress_dev")

    def fqz_peek(self, d_in, in_off, in_size, raw_size, status, max_in_size):
        """rans4x16_hip_fqz_peek_dev: the stored size of every fqzcomp_qual stream."""
        t = self.torch
        assert d_in.dtype == t.uint8 and in_off.dtype == t.int64 and in_size.dtype == t.int32
        assert raw_size.dtype == t.int32 and status.dtype == t.int32
        rc = self.L.rans4x16_hip_fqz_peek_dev(self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
                                              raw_size.data_ptr(), status.data_ptr(), int(max_in_size), self._stream())
        self._check(rc, "fqz_peek_dev")

    def set_fqz_limits(self, max_slots=0, max_sym=0):
        """rans4x16_hip_set_fqz_limits: the model slots in flight at most (0: 1024) and the largest max_sym a slot holds
        (0: 255)."""
        if self.L.rans4x16_hip_set_fqz_limits(self.ctx.h, int(max_slots), int(max_sym)) != 0:
            raise ValueError("set_fqz_limits: " + self.ctx.error())

    # ---- fqzcomp_qual encoding (include/rans4x16_hip.h part 2j) -------------------------------------------------------
    def fqz_compress(self, d_in, in_off, in_size, d_params, par_off, par_size, d_len, d_flags, rec_off, nrec,
                     d_out, out_off, out_cap, out_size, status, max_in_size, max_params_size, max_records):
        """rans4x16_hip_fqz_compress_dev: per block the qualities, the parameter bytes (uint8 at par_off, int64, of par_size,
        int32) and the records (nrec, int32, lengths and flags as int32 entries from rec_off, int64, in d_len / d_flags),
        fqzcomp_qual streams out.  Enqueues only."""
        t = self.torch
        self._slot_args(d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status)
        assert d_params.dtype == t.uint8 and par_off.dtype == t.int64 and rec_off.dtype == t.int64
        assert par_size.dtype == t.int32 and nrec.dtype == t.int32 and d_len.dtype == t.int32 and d_flags.dtype == t.int32
        rc = self.L.rans4x16_hip_fqz_compress_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_params.data_ptr(), par_off.data_ptr(), par_size.data_ptr(),
            d_len.data_ptr(), d_flags.data_ptr(), rec_off.data_ptr(), nrec.data_ptr(),
            d_out.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(), out_size.data_ptr(), status.data_ptr(),
            int(max_in_size), int(max_params_size), int(max_records), self._stream())
        self._check(rc, "fqz_compress_dev")

    # ---- fqzcomp_qual encoding: the parameter choice on the device (include/rans4x16_hip.h part 2k) -----------------------
    def set_fqz_pick(self, mode=0, guard_bits=0):
        """rans4x16_hip_set_fqz_pick: mode 1 makes fqz_compress_batch on this context pick on the device; guard_bits
        widens the guard of every device pick by 2^guard_bits."""
        if self.L.rans4x16_hip_set_fqz_pick(self.ctx.h, int(mode), int(guard_bits)) != 0:
            raise ValueError("set_fqz_pick: " + self.ctx.error())

    def _pick_args(self, d_in, in_off, in_size, d_len, d_flags, rec_off, nrec, d_strat):
        t = self.torch
        assert d_in.dtype == t.uint8 and in_off.dtype == t.int64 and in_size.dtype == t.int32 and rec_off.dtype == t.int64
        assert nrec.dtype == t.int32 and d_len.dtype == t.int32 and d_flags.dtype == t.int32
        assert d_strat is None or d_strat.dtype == t.int32

    def fqz_pick(self, d_in, in_off, in_size, d_len, d_flags, rec_off, nrec, d_params, par_off, par_cap, par_size,
                 d_len_out, d_flags_out, status, max_in_size, max_records, vers=4, strat=0, d_strat=None):
        """rans4x16_hip_fqz_pick_dev: per block the qualities and the records (as in fqz_compress) -> its parameter bytes
        (uint8 at par_off, int64, up to par_cap, int32; the size in par_size) and its slice as the pick leaves it in
        d_len_out / d_flags_out (int32; may be d_len / d_flags).  d_strat: per-block strategies (int32).  Enqueues only."""
        t = self.torch
        self._pick_args(d_in, in_off, in_size, d_len, d_flags, rec_off, nrec, d_strat)
        assert d_params.dtype == t.uint8 and par_off.dtype == t.int64 and par_cap.dtype == t.int32 and par_size.dtype == t.int32
        assert d_len_out.dtype == t.int32 and d_flags_out.dtype == t.int32 and status.dtype == t.int32
        rc = self.L.rans4x16_hip_fqz_pick_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_len.data_ptr(), d_flags.data_ptr(), rec_off.data_ptr(), nrec.data_ptr(),
            int(vers), int(strat), d_strat.data_ptr() if d_strat is not None else None,
            d_params.data_ptr(), par_off.data_ptr(), par_cap.data_ptr(), par_size.data_ptr(),
            d_len_out.data_ptr(), d_flags_out.data_ptr(), status.data_ptr(),
            int(max_in_size), int(max_records), self._stream())
        self._check(rc, "fqz_pick_dev")

    def fqz_compress_pick(self, d_in, in_off, in_size, d_len, d_flags, rec_off, nrec, d_out, out_off, out_cap, out_size,
                          status, max_in_size, max_records, vers=4, strat=0, d_strat=None):
        """rans4x16_hip_fqz_compress_pick_dev: the device pick and fqz_compress in one call; the caller's records are only
        read.  Enqueues only."""
        self._slot_args(d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status)
        self._pick_args(d_in, in_off, in_size, d_len, d_flags, rec_off, nrec, d_strat)
        rc = self.L.rans4x16_hip_fqz_compress_pick_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_len.data_ptr(), d_flags.data_ptr(), rec_off.data_ptr(), nrec.data_ptr(),
            int(vers), int(strat), d_strat.data_ptr() if d_strat is not None else None,
            d_out.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(), out_size.data_ptr(), status.data_ptr(),
            int(max_in_size), int(max_records), self._stream())
        self._check(rc, "fqz_compress_pick_dev")

    # ---- fqzcomp_qual encoding: best of several strategies (include/rans4x16_hip.h part 2l) -----------------------------
    def fqz_compress_best(self, d_in, in_off, in_size, d_len, d_flags, rec_off, nrec, d_out, out_off, out_cap, out_size,
                          status, strats, max_in_size, max_records, vers=4, chosen=None, d_len_out=None):
        """rans4x16_hip_fqz_compress_best_dev: fqz_compress_pick under every strategy of `strats` (a host list), the smallest
        stream into the slot; chosen (int32): the winner's index into strats, d_len_out (int32): the lengths as the fix-ups
        leave them.  Enqueues only."""
        t = self.torch
        self._slot_args(d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status)
        self._pick_args(d_in, in_off, in_size, d_len, d_flags, rec_off, nrec, None)
        assert chosen is None or chosen.dtype == t.int32
        assert d_len_out is None or d_len_out.dtype == t.int32
        st = (C.c_int * max(len(strats), 1))(*[int(v) for v in strats])
        rc = self.L.rans4x16_hip_fqz_compress_best_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_len.data_ptr(), d_flags.data_ptr(), rec_off.data_ptr(), nrec.data_ptr(), int(vers), len(strats), st,
            d_out.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(), out_size.data_ptr(), status.data_ptr(),
            chosen.data_ptr() if chosen is not None else None, d_len_out.data_ptr() if d_len_out is not None else None,
            int(max_in_size), int(max_records), self._stream())
        self._check(rc, "fqz_compress_best_dev")

    def fqz_compress_best_packed(self, d_in, in_off, in_size, d_len, d_flags, rec_off, nrec, d_out, out_off, out_size, status,
                                 strats, max_in_size, max_records, vers=4, chosen=None, d_len_out=None, out_capacity=None):
        """rans4x16_hip_fqz_compress_best_packed_dev: the same with the winners back to back in d_out and out_off (int64,
        n + 1) written on the device.  d_out None (with out_capacity 0 or None) is the sizing pass."""
        t = self.torch
        assert d_out is None or d_out.dtype == t.uint8
        assert out_off.dtype == t.int64 and out_off.numel() == in_off.numel() + 1
        assert out_size.dtype == t.int32 and status.dtype == t.int32
        self._pick_args(d_in, in_off, in_size, d_len, d_flags, rec_off, nrec, None)
        assert chosen is None or chosen.dtype == t.int32
        assert d_len_out is None or d_len_out.dtype == t.int32
        room = d_out.numel() if d_out is not None else 0
        cap = room if out_capacity is None else int(out_capacity)
        assert cap <= room
        st = (C.c_int * max(len(strats), 1))(*[int(v) for v in strats])
        rc = self.L.rans4x16_hip_fqz_compress_best_packed_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_len.data_ptr(), d_flags.data_ptr(), rec_off.data_ptr(), nrec.data_ptr(), int(vers), len(strats), st,
            d_out.data_ptr() if d_out is not None else None, cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(),
            chosen.data_ptr() if chosen is not None else None, d_len_out.data_ptr() if d_len_out is not None else None,
            int(max_in_size), int(max_records), self._stream())
        self._check(rc, "fqz_compress_best_packed_dev")

    def fqz_best_chunk_blocks(self, n, k, max_in_size, max_records):
        """rans4x16_hip_fqz_best_chunk_blocks: the blocks per chunk fqz_compress_best plans for these arguments."""
        rc = self.L.rans4x16_hip_fqz_best_chunk_blocks(self.ctx.h, int(n), int(k), int(max_in_size), int(max_records))
        if rc < 0:
            raise RuntimeError("fqz_best_chunk_blocks: " + self.ctx.error())
        return rc

    # ---- what the methods share: the dtypes of either form's arrays, and the end of every call ----------------------
    def _slot_args(self, d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status):
        t = self.torch
        assert d_in.dtype == t.uint8 and d_out.dtype == t.uint8
        assert in_off.dtype == t.int64 and out_off.dtype == t.int64
        assert in_size.dtype == t.int32 and out_cap.dtype == t.int32
        assert out_size.dtype == t.int32 and status.dtype == t.int32

    def _check(self, rc, name):
        if rc != 0:
            raise RuntimeError(name + ": " + self.ctx.error())

    # ---- packed calls (include/rans4x16_hip.h part 2a): one dense arena, offsets written by the device ----------
    def _packed_args(self, d_in, in_off, in_size, d_out, out_off, out_size, status):
        t = self.torch
        assert d_in.dtype == t.uint8 and d_out.dtype == t.uint8
        assert in_off.dtype == t.int64 and in_size.dtype == t.int32
        assert out_off.dtype == t.int64 and out_off.numel() == in_off.numel() + 1
        assert out_size.dtype == t.int32 and status.dtype == t.int32

    def compress_packed(self, d_in, in_off, in_size, d_out, out_off, out_size, status, order, max_in_size,
                        d_order=None, total_in_size=0, out_capacity=None):
        """rans4x16_hip_compress_packed_dev: block i at d_out[out_off[i]:out_off[i + 1]]; out_off (int64, n + 1 entries) is
        written by the call, out_off[n] is what the batch needs.  out_capacity defaults to d_out's size."""
        self._packed_args(d_in, in_off, in_size, d_out, out_off, out_size, status)
        cap = d_out.numel() if out_capacity is None else int(out_capacity)
        assert cap <= d_out.numel()
        rc = self.L.rans4x16_hip_compress_packed_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr(), cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(), int(order),
            d_order.data_ptr() if d_order is not None else None, int(max_in_size), int(total_in_size), self._stream())
        self._check(rc, "compress_packed_dev")

    def compress_best_packed(self, d_in, in_off, in_size, d_out, out_off, out_size, status, methods, max_in_size,
                             chosen=None, total_in_size=0, out_capacity=None):
        """rans4x16_hip_compress_best_packed_dev: compress_best with the winners back to back in d_out."""
        self._packed_args(d_in, in_off, in_size, d_out, out_off, out_size, status)
        assert chosen is None or chosen.dtype == self.torch.int32
        cap = d_out.numel() if out_capacity is None else int(out_capacity)
        assert cap <= d_out.numel()
        meth = _methods(methods)
        rc = self.L.rans4x16_hip_compress_best_packed_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr(), cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(), len(methods), meth,
            chosen.data_ptr() if chosen is not None else None, int(max_in_size), int(total_in_size), self._stream())
        self._check(rc, "compress_best_packed_dev")

    def arith_compress_best_packed(self, d_in, in_off, in_size, d_out, out_off, out_size, status, methods, max_in_size,
                                   chosen=None, total_in_size=0, out_capacity=None):
        """rans4x16_hip_arith_compress_best_packed_dev: compress_best_packed for the adaptive arithmetic coder.  d_out None
        (with out_capacity 0 or None) is the sizing pass."""
        t = self.torch
        assert d_in.dtype == t.uint8 and (d_out is None or d_out.dtype == t.uint8)
        assert in_off.dtype == t.int64 and in_size.dtype == t.int32
        assert out_off.dtype == t.int64 and out_off.numel() == in_off.numel() + 1
        assert out_size.dtype == t.int32 and status.dtype == t.int32
        assert chosen is None or chosen.dtype == t.int32
        room = d_out.numel() if d_out is not None else 0
        cap = room if out_capacity is None else int(out_capacity)
        assert cap <= room
        meth = _methods(methods)
        rc = self.L.rans4x16_hip_arith_compress_best_packed_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr() if d_out is not None else None, cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(),
            len(methods), meth, chosen.data_ptr() if chosen is not None else None, int(max_in_size), int(total_in_size),
            self._stream())
        self._check(rc, "arith_compress_best_packed_dev")

    def arith_best_chunk_blocks(self, n, methods, max_in_size, total_in_size=0):
        """rans4x16_hip_arith_best_chunk_blocks: the blocks per chunk arith_compress_best_packed plans for these arguments."""
        meth = _methods(methods)
        rc = self.L.rans4x16_hip_arith_best_chunk_blocks(self.ctx.h, int(n), len(methods), meth, int(max_in_size), int(total_in_size))
        if rc < 0:
            raise RuntimeError("arith_best_chunk_blocks: " + self.ctx.error())
        return rc

    # ---- best of several methods across codecs (include/rans4x16_hip.h part 2m) ---------------------------------
    def compress_best_any_packed(self, d_in, in_off, in_size, d_out, out_off, out_size, status, methods, max_in_size,
                                 chosen=None, total_in_size=0, out_capacity=None):
        """rans4x16_hip_compress_best_any_packed_dev: compress_best_packed over a list of tagged methods (CODEC_ARITH | order
        for arith_dynamic, a plain order word for rANS 4x16); chosen gets the winner's tagged word.  d_out None (with
        out_capacity 0 or None) is the sizing pass."""
        t = self.torch
        assert d_in.dtype == t.uint8 and (d_out is None or d_out.dtype == t.uint8)
        assert in_off.dtype == t.int64 and in_size.dtype == t.int32
        assert out_off.dtype == t.int64 and out_off.numel() == in_off.numel() + 1
        assert out_size.dtype == t.int32 and status.dtype == t.int32
        assert chosen is None or chosen.dtype == t.int32
        room = d_out.numel() if d_out is not None else 0
        cap = room if out_capacity is None else int(out_capacity)
        assert cap <= room
        meth = _methods(methods)
        rc = self.L.rans4x16_hip_compress_best_any_packed_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr() if d_out is not None else None, cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(),
            len(methods), meth, chosen.data_ptr() if chosen is not None else None, int(max_in_size), int(total_in_size),
            self._stream())
        self._check(rc, "compress_best_any_packed_dev")

    def best_any_chunk_blocks(self, n, methods, max_in_size, total_in_size=0):
        """rans4x16_hip_best_any_chunk_blocks: the blocks per chunk compress_best_any_packed plans for these arguments."""
        meth = _methods(methods)
        rc = self.L.rans4x16_hip_best_any_chunk_blocks(self.ctx.h, int(n), len(methods), meth, int(max_in_size), int(total_in_size))
        if rc < 0:
            raise RuntimeError("best_any_chunk_blocks: " + self.ctx.error())
        return rc

    def uncompress_any_packed(self, d_in, in_off, in_size, method, d_out, out_off, out_size, status, max_in_size, max_out_size,
                              nosz_size=None, out_capacity=None):
        """rans4x16_hip_uncompress_any_packed_dev: uncompress_packed for an arena that mixes both codecs; method (int32
        tensor: compress_best_any_packed's chosen goes straight in) says which decodes block i."""
        t = self.torch
        n = in_size.numel()
        assert d_in.dtype == t.uint8 and (d_out is None or d_out.dtype == t.uint8)
        assert in_off.dtype == t.int64 and in_off.numel() >= n and in_size.dtype == t.int32
        assert method.dtype == t.int32 and method.numel() == n
        assert out_off.dtype == t.int64 and out_off.numel() == n + 1
        assert out_size.dtype == t.int32 and status.dtype == t.int32
        assert nosz_size is None or (nosz_size.dtype == t.int32 and nosz_size.numel() == n)
        room = d_out.numel() if d_out is not None else 0
        cap = room if out_capacity is None else int(out_capacity)
        assert cap <= room
        rc = self.L.rans4x16_hip_uncompress_any_packed_dev(
            self.ctx.h, n, d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(), method.data_ptr(),
            d_out.data_ptr() if d_out is not None else None, cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(),
            nosz_size.data_ptr() if nosz_size is not None else None, int(max_in_size), int(max_out_size), self._stream())
        self._check(rc, "uncompress_any_packed_dev")

    # ---- quality blocks: best across rANS 4x16, arith_dynamic and fqzcomp_qual (include/rans4x16_hip.h part 2n) ----------
    def compress_best_qual_packed(self, d_in, in_off, in_size, d_len, d_flags, rec_off, nrec, d_out, out_off, out_size, status,
                                  methods, max_in_size, max_records, vers=4, chosen=None, d_len_out=None, total_in_size=0,
                                  out_capacity=None):
        """rans4x16_hip_compress_best_qual_packed_dev: fqz_compress_best_packed's arguments under a list of tagged methods (a
        plain order word for rANS 4x16, CODEC_ARITH | order, CODEC_FQZ | strat); chosen gets the winner's tagged word,
        d_len_out the lengths of the blocks fqzcomp_qual won.  A list without a CODEC_FQZ entry takes None for the four
        record tensors.  d_out None (with out_capacity 0 or None) is the sizing pass."""
        t = self.torch
        assert d_in.dtype == t.uint8 and (d_out is None or d_out.dtype == t.uint8)
        assert in_off.dtype == t.int64 and in_size.dtype == t.int32
        assert out_off.dtype == t.int64 and out_off.numel() == in_off.numel() + 1
        assert out_size.dtype == t.int32 and status.dtype == t.int32
        assert all(x is None or x.dtype == t.int32 for x in (d_len, d_flags, nrec, chosen, d_len_out))
        assert rec_off is None or rec_off.dtype == t.int64
        room = d_out.numel() if d_out is not None else 0
        cap = room if out_capacity is None else int(out_capacity)
        assert cap <= room
        meth = _methods(methods)
        ptr = lambda x: x.data_ptr() if x is not None else None
        rc = self.L.rans4x16_hip_compress_best_qual_packed_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            ptr(d_len), ptr(d_flags), ptr(rec_off), ptr(nrec), int(vers), len(methods), meth,
            ptr(d_out), cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(), ptr(chosen), ptr(d_len_out),
            int(max_in_size), int(max_records), int(total_in_size), self._stream())
        self._check(rc, "compress_best_qual_packed_dev")

    def best_qual_chunk_blocks(self, n, methods, max_in_size, max_records, total_in_size=0):
        """rans4x16_hip_best_qual_chunk_blocks: the blocks per chunk compress_best_qual_packed plans for these arguments."""
        meth = _methods(methods)
        rc = self.L.rans4x16_hip_best_qual_chunk_blocks(self.ctx.h, int(n), len(methods), meth, int(max_in_size), int(max_records),
                                                        int(total_in_size))
        if rc < 0:
            raise RuntimeError("best_qual_chunk_blocks: " + self.ctx.error())
        return rc

    def uncompress_qual_packed(self, d_in, in_off, in_size, method, d_out, out_off, out_size, status, max_in_size, max_out_size,
                               nosz_size=None, out_capacity=None, d_len=None, len_off=None, len_cap=None, nrec=None):
        """rans4x16_hip_uncompress_qual_packed_dev: uncompress_any_packed for an arena that mixes the three codecs, with
        fqz_uncompress's four optional length arguments (written for the CODEC_FQZ blocks; nrec is 0 for the others)."""
        t = self.torch
        n = in_size.numel()
        assert d_in.dtype == t.uint8 and (d_out is None or d_out.dtype == t.uint8)
        assert in_off.dtype == t.int64 and in_off.numel() >= n and in_size.dtype == t.int32
        assert method.dtype == t.int32 and method.numel() == n
        assert out_off.dtype == t.int64 and out_off.numel() == n + 1
        assert out_size.dtype == t.int32 and status.dtype == t.int32
        assert nosz_size is None or (nosz_size.dtype == t.int32 and nosz_size.numel() == n)
        assert d_len is None or (d_len.dtype == t.int32 and len_off.dtype == t.int64 and len_cap.dtype == t.int32)
        assert nrec is None or nrec.dtype == t.int32
        room = d_out.numel() if d_out is not None else 0
        cap = room if out_capacity is None else int(out_capacity)
        assert cap <= room
        ptr = lambda x: x.data_ptr() if x is not None else None
        rc = self.L.rans4x16_hip_uncompress_qual_packed_dev(
            self.ctx.h, n, d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(), method.data_ptr(),
            ptr(d_out), cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(), ptr(nosz_size),
            ptr(d_len), ptr(len_off), ptr(len_cap), ptr(nrec), int(max_in_size), int(max_out_size), self._stream())
        self._check(rc, "uncompress_qual_packed_dev")

    def set_tok3_arith(self, mode):
        """rans4x16_hip_set_tok3_arith: 0, TOK3_ARITH_DECODE (1), TOK3_ARITH_ENCODE (2) or both; returns the previous mode."""
        return set_tok3_arith(mode, self.ctx)

    def peek(self, d_in, in_off, in_size, fmt, raw_size, status, max_in_size):
        """rans4x16_hip_peek_dev: first byte (fmt, int32) and stored uncompressed size (raw_size, int32 holding the
        unsigned value; -1 = the stream carries none) of every block."""
        t = self.torch
        assert d_in.dtype == t.uint8 and in_off.dtype == t.int64 and in_size.dtype == t.int32
        assert fmt.dtype == t.int32 and raw_size.dtype == t.int32 and status.dtype == t.int32
        rc = self.L.rans4x16_hip_peek_dev(self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
                                          fmt.data_ptr(), raw_size.data_ptr(), status.data_ptr(), int(max_in_size), self._stream())
        self._check(rc, "peek_dev")

    def uncompress_packed(self, d_in, in_off, in_size, d_out, out_off, out_size, status, max_in_size, max_out_size,
                          nosz_size=None, out_capacity=None):
        """rans4x16_hip_uncompress_packed_dev: every block decoded to d_out[out_off[i]:out_off[i + 1]], the sizes taken from
        the streams (nosz_size: int32 tensor with the sizes of X_NOSZ blocks, optional).  in_off may have n or n + 1
        entries (compress_packed's out_off goes straight in); the block count is in_size's."""
        t = self.torch
        n = in_size.numel()
        assert d_in.dtype == t.uint8 and d_out.dtype == t.uint8
        assert in_off.dtype == t.int64 and in_off.numel() >= n and in_size.dtype == t.int32
        assert out_off.dtype == t.int64 and out_off.numel() == n + 1
        assert out_size.dtype == t.int32 and status.dtype == t.int32
        assert nosz_size is None or (nosz_size.dtype == t.int32 and nosz_size.numel() == n)
        cap = d_out.numel() if out_capacity is None else int(out_capacity)
        assert cap <= d_out.numel()
        rc = self.L.rans4x16_hip_uncompress_packed_dev(
            self.ctx.h, n, d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr(), cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(),
            nosz_size.data_ptr() if nosz_size is not None else None, int(max_in_size), int(max_out_size), self._stream())
        self._check(rc, "uncompress_packed_dev")

    # ---- tok3 column containers (include/rans4x16_hip.h part 2c) -------------------------------------------------
    def tok3_pack(self, blk_first, d_in, col_off, col_size, col_id, last_start, nreads, d_out, out_off, out_size, status,
                  methods, max_col_size, chosen=None, total_col_size=0, out_capacity=None):
        """rans4x16_hip_tok3_pack_dev: the columns col_off / col_size / col_id (int64 / int32 / int32) of the blocks
        blk_first (int32, nblk + 1 entries) compressed with the best of `methods` and framed into one container per block
        at d_out[out_off[b]:out_off[b + 1]].  d_out None: the sizing pass."""
        t = self.torch
        nblk, n = blk_first.numel() - 1, col_off.numel()
        assert blk_first.dtype == t.int32 and col_off.dtype == t.int64 and col_size.dtype == t.int32 and col_id.dtype == t.int32
        assert col_size.numel() == n and col_id.numel() == n
        assert last_start.dtype == t.int32 and nreads.dtype == t.int32 and last_start.numel() == nblk and nreads.numel() == nblk
        assert out_off.dtype == t.int64 and out_off.numel() == nblk + 1
        assert out_size.dtype == t.int32 and status.dtype == t.int32 and out_size.numel() == nblk and status.numel() == nblk
        assert chosen is None or (chosen.dtype == t.int32 and chosen.numel() == n)
        assert d_in.dtype == t.uint8 and (d_out is None or d_out.dtype == t.uint8)
        cap = (d_out.numel() if d_out is not None else 0) if out_capacity is None else int(out_capacity)
        assert cap <= (d_out.numel() if d_out is not None else 0)
        meth = _methods(methods)
        rc = self.L.rans4x16_hip_tok3_pack_dev(
            self.ctx.h, nblk, n, blk_first.data_ptr(), d_in.data_ptr(), col_off.data_ptr(), col_size.data_ptr(),
            col_id.data_ptr(), last_start.data_ptr(), nreads.data_ptr(), d_out.data_ptr() if d_out is not None else None, cap,
            out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(), len(methods), meth,
            chosen.data_ptr() if chosen is not None else None, int(max_col_size), int(total_col_size), self._stream())
        self._check(rc, "tok3_pack_dev")

    def tok3_unpack(self, d_in, in_off, in_size, d_out, out_off, out_size, status, ncol, last_start, nreads,
                    col_id, col_off, col_size, max_columns, max_in_size, max_col_size, out_capacity=None):
        """rans4x16_hip_tok3_unpack_dev: every container walked and its columns decoded back to back into
        d_out[out_off[b]:out_off[b + 1]]; col_id / col_off / col_size (int32 / int64 / int32, nblk x max_columns) are the
        directory of the columns.  d_out None: the sizing pass."""
        t = self.torch
        nblk = in_size.numel()
        assert d_in.dtype == t.uint8 and (d_out is None or d_out.dtype == t.uint8)
        assert in_off.dtype == t.int64 and in_off.numel() >= nblk and in_size.dtype == t.int32
        assert out_off.dtype == t.int64 and out_off.numel() == nblk + 1
        for x in (out_size, status, ncol, last_start, nreads):
            assert x.dtype == t.int32 and x.numel() == nblk
        assert col_id.dtype == t.int32 and col_off.dtype == t.int64 and col_size.dtype == t.int32
        for x in (col_id, col_off, col_size):
            assert x.numel() == nblk * int(max_columns)
        cap = (d_out.numel() if d_out is not None else 0) if out_capacity is None else int(out_capacity)
        assert cap <= (d_out.numel() if d_out is not None else 0)
        rc = self.L.rans4x16_hip_tok3_unpack_dev(
            self.ctx.h, nblk, d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr() if d_out is not None else None, cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(),
            ncol.data_ptr(), last_start.data_ptr(), nreads.data_ptr(), col_id.data_ptr(), col_off.data_ptr(), col_size.data_ptr(),
            int(max_columns), int(max_in_size), int(max_col_size), self._stream())
        self._check(rc, "tok3_unpack_dev")

    # ---- tok3 name decoding (include/rans4x16_hip.h part 2d) ---------------------------------------------------------
    def _names_out(self, nblk, d_out, out_off, out_size, nnames, status, name_start, max_names, out_capacity):
        t = self.torch
        assert d_out is None or d_out.dtype == t.uint8
        assert out_off.dtype == t.int64 and out_off.numel() == nblk + 1
        for x in (out_size, nnames, status):
            assert x.dtype == t.int32 and x.numel() == nblk
        assert name_start is None or (name_start.dtype == t.int32 and name_start.numel() == nblk * int(max_names))
        cap = (d_out.numel() if d_out is not None else 0) if out_capacity is None else int(out_capacity)
        assert cap <= (d_out.numel() if d_out is not None else 0)
        return cap

    def tok3_names(self, d_cols, col_id, col_off, col_size, ncol, last_start, nreads, d_out, out_off, out_size, nnames, status,
                   max_columns, max_names, max_tokens=128, blk_status=None, name_start=None, out_capacity=None):
        """rans4x16_hip_tok3_names_dev: the columns tok3_unpack left in d_cols (its directory col_id / col_off / col_size and
        ncol / last_start / nreads go straight in, its status as blk_status) decoded to NUL-separated read names at
        d_out[out_off[b]:out_off[b + 1]]; name_start (int32, nblk x max_names, optional): where every name starts inside
        its block.  d_out None: the sizing pass."""
        t = self.torch
        nblk = ncol.numel()
        assert d_cols.dtype == t.uint8
        assert col_id.dtype == t.int32 and col_off.dtype == t.int64 and col_size.dtype == t.int32
        for x in (col_id, col_off, col_size):
            assert x.numel() == nblk * int(max_columns)
        for x in (ncol, last_start, nreads):
            assert x.dtype == t.int32 and x.numel() == nblk
        assert blk_status is None or (blk_status.dtype == t.int32 and blk_status.numel() == nblk)
        cap = self._names_out(nblk, d_out, out_off, out_size, nnames, status, name_start, max_names, out_capacity)
        rc = self.L.rans4x16_hip_tok3_names_dev(
            self.ctx.h, nblk, d_cols.data_ptr(), d_cols.numel(), col_id.data_ptr(), col_off.data_ptr(), col_size.data_ptr(),
            ncol.data_ptr(), last_start.data_ptr(), nreads.data_ptr(), blk_status.data_ptr() if blk_status is not None else None,
            d_out.data_ptr() if d_out is not None else None, cap, out_off.data_ptr(), out_size.data_ptr(), nnames.data_ptr(),
            status.data_ptr(), name_start.data_ptr() if name_start is not None else None,
            int(max_columns), int(max_names), int(max_tokens), self._stream())
        self._check(rc, "tok3_names_dev")

    def tok3_decode_names(self, d_in, in_off, in_size, d_out, out_off, out_size, nnames, status, max_columns, max_in_size,
                          max_col_size, max_names, max_tokens=128, total_col_size=0, name_start=None, out_capacity=None):
        """rans4x16_hip_tok3_decode_names_dev: every container walked, its columns decoded and its read names written,
        NUL-separated, at d_out[out_off[b]:out_off[b + 1]] - tok3_unpack and tok3_names in one call, the columns kept in an
        arena of the context (total_col_size: their bytes, 0 = unknown).  d_out None: the sizing pass."""
        t = self.torch
        nblk = in_size.numel()
        assert d_in.dtype == t.uint8 and in_off.dtype == t.int64 and in_off.numel() >= nblk and in_size.dtype == t.int32
        cap = self._names_out(nblk, d_out, out_off, out_size, nnames, status, name_start, max_names, out_capacity)
        rc = self.L.rans4x16_hip_tok3_decode_names_dev(
            self.ctx.h, nblk, d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr() if d_out is not None else None, cap, out_off.data_ptr(), out_size.data_ptr(), nnames.data_ptr(),
            status.data_ptr(), name_start.data_ptr() if name_start is not None else None,
            int(max_columns), int(max_in_size), int(max_col_size), int(max_names), int(max_tokens), int(total_col_size),
            self._stream())
        self._check(rc, "tok3_decode_names_dev")

    # ---- tok3 name encoding (include/rans4x16_hip.h part 2e) ---------------------------------------------------------
    def tok3_tokenise(self, d_in, in_off, in_size, d_cols, cols_off, cols_size, status, blk_first, col_id, col_off, col_size,
                      last_start, nreads, max_in_size, max_names, max_name_len, max_columns, max_tokens=128, total_in_size=0,
                      search_slots=0, col_capacity=None):
        """rans4x16_hip_tok3_tokenise_dev: the name blocks d_in[in_off[b]:in_off[b] + in_size[b]] (a name ends at any byte
        <= '\\n') turned into their token columns at d_cols[cols_off[b]:cols_off[b + 1]]; blk_first (int32, nblk + 1) and
        col_id / col_off / col_size (int32 / int64 / int32, nblk x max_columns) are the dense directory tok3_pack takes,
        last_start / nreads its header values.  d_cols None: the sizing pass.  search_slots 1: the exact search alone."""
        t = self.torch
        nblk = in_size.numel()
        assert d_in.dtype == t.uint8 and in_off.dtype == t.int64 and in_off.numel() >= nblk and in_size.dtype == t.int32
        assert d_cols is None or d_cols.dtype == t.uint8
        assert cols_off.dtype == t.int64 and cols_off.numel() == nblk + 1
        assert blk_first.dtype == t.int32 and blk_first.numel() == nblk + 1
        for x in (cols_size, status, last_start, nreads):
            assert x.dtype == t.int32 and x.numel() == nblk
        assert col_id.dtype == t.int32 and col_off.dtype == t.int64 and col_size.dtype == t.int32
        for x in (col_id, col_off, col_size):
            assert x.numel() == nblk * int(max_columns)
        cap = (d_cols.numel() if d_cols is not None else 0) if col_capacity is None else int(col_capacity)
        assert cap <= (d_cols.numel() if d_cols is not None else 0)
        rc = self.L.rans4x16_hip_tok3_tokenise_dev(
            self.ctx.h, nblk, d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_cols.data_ptr() if d_cols is not None else None, cap, cols_off.data_ptr(), cols_size.data_ptr(), status.data_ptr(),
            blk_first.data_ptr(), col_id.data_ptr(), col_off.data_ptr(), col_size.data_ptr(), last_start.data_ptr(),
            nreads.data_ptr(), int(max_in_size), int(max_names), int(max_name_len), int(max_tokens), int(max_columns),
            int(total_in_size), int(search_slots), self._stream())
        self._check(rc, "tok3_tokenise_dev")

    def tok3_encode_names(self, d_in, in_off, in_size, d_out, out_off, out_size, status, methods, max_in_size, max_names,
                          max_name_len, max_columns, max_tokens=128, max_col_size=0, total_in_size=0, search_slots=0,
                          chosen=None, blk_first=None, out_capacity=None):
        """rans4x16_hip_tok3_encode_names_dev: the name blocks d_in[in_off[b]:in_off[b] + in_size[b]] tokenised, their
        columns compressed with the best of `methods` and framed into one container per block at
        d_out[out_off[b]:out_off[b + 1]] - tok3_tokenise and tok3_pack in one call, the columns kept in an arena of the
        context.  chosen (int32, nblk x max_columns) / blk_first (int32, nblk + 1): optional.  d_out None: the sizing pass."""
        t = self.torch
        nblk = in_size.numel()
        assert d_in.dtype == t.uint8 and in_off.dtype == t.int64 and in_off.numel() >= nblk and in_size.dtype == t.int32
        assert d_out is None or d_out.dtype == t.uint8
        assert out_off.dtype == t.int64 and out_off.numel() == nblk + 1
        assert out_size.dtype == t.int32 and status.dtype == t.int32 and out_size.numel() == nblk and status.numel() == nblk
        assert chosen is None or (chosen.dtype == t.int32 and chosen.numel() == nblk * int(max_columns))
        assert blk_first is None or (blk_first.dtype == t.int32 and blk_first.numel() == nblk + 1)
        cap = (d_out.numel() if d_out is not None else 0) if out_capacity is None else int(out_capacity)
        assert cap <= (d_out.numel() if d_out is not None else 0)
        meth = _methods(methods)
        rc = self.L.rans4x16_hip_tok3_encode_names_dev(
            self.ctx.h, nblk, d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr() if d_out is not None else None, cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(),
            len(methods), meth, chosen.data_ptr() if chosen is not None else None,
            blk_first.data_ptr() if blk_first is not None else None, int(max_in_size), int(max_names), int(max_name_len),
            int(max_tokens), int(max_columns), int(max_col_size), int(total_in_size), int(search_slots), self._stream())
        self._check(rc, "tok3_encode_names_dev")

    # ---- rANS 4x8 (CRAM 3.0), include/rans4x8_hip.h part 2a: the same surface, every result assembled in place -------
    def compress_packed_4x8(self, d_in, in_off, in_size, d_out, out_off, out_size, status, order, max_in_size,
                            d_order=None, out_capacity=None):
        """rans4x8_hip_compress_packed_dev: block i at d_out[out_off[i]:out_off[i + 1]]; out_off (int64, n + 1 entries) is
        written by the call, out_off[n] is what the batch needs.  out_capacity defaults to d_out's size."""
        self._packed_args(d_in, in_off, in_size, d_out, out_off, out_size, status)
        cap = d_out.numel() if out_capacity is None else int(out_capacity)
        assert cap <= d_out.numel()
        rc = self.L.rans4x8_hip_compress_packed_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr(), cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(), int(order),
            d_order.data_ptr() if d_order is not None else None, int(max_in_size), self._stream())
        self._check(rc, "rans4x8 compress_packed_dev")

    def compress_best_4x8(self, d_in, in_off, in_size, d_out, out_off, out_size, status, methods, max_in_size,
                          chosen=None, packed=False, out_cap=None, out_capacity=None):
        """Every block with each of `methods` (one or two of 0 / 1), the smaller result kept, the first on a tie; `chosen`
        (int32 tensor, optional) gets the winner's index into `methods`, -1 for a failed block.
        packed=False: rans4x8_hip_compress_best_dev, the winner in its slot (out_off: n entries, read; out_cap: int32).
        packed=True: rans4x8_hip_compress_best_packed_dev, the winners back to back (out_off: n + 1 entries, written)."""
        t = self.torch
        assert chosen is None or chosen.dtype == t.int32
        meth = _methods(methods)
        ch = chosen.data_ptr() if chosen is not None else None
        if packed:
            self._packed_args(d_in, in_off, in_size, d_out, out_off, out_size, status)
            cap = d_out.numel() if out_capacity is None else int(out_capacity)
            assert cap <= d_out.numel()
            rc = self.L.rans4x8_hip_compress_best_packed_dev(
                self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
                d_out.data_ptr(), cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(), len(methods), meth, ch,
                int(max_in_size), self._stream())
        else:
            assert out_cap is not None and out_off.numel() == in_off.numel()
            self._slot_args(d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status)
            rc = self.L.rans4x8_hip_compress_best_dev(
                self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
                d_out.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(), out_size.data_ptr(), status.data_ptr(),
                len(methods), meth, ch, int(max_in_size), self._stream())
        self._check(rc, "rans4x8 compress_best%s_dev" % ("_packed" if packed else ""))

    def peek_4x8(self, d_in, in_off, in_size, fmt, raw_size, status, max_in_size):
        """rans4x8_hip_peek_dev: byte 0 (fmt, int32; -1 = none) and bytes 5..8 (raw_size, int32 holding the unsigned value;
        -1 = fewer than 9 bytes) of every block."""
        t = self.torch
        assert d_in.dtype == t.uint8 and in_off.dtype == t.int64 and in_size.dtype == t.int32
        assert fmt.dtype == t.int32 and raw_size.dtype == t.int32 and status.dtype == t.int32
        rc = self.L.rans4x8_hip_peek_dev(self.ctx.h, in_size.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
                                         fmt.data_ptr(), raw_size.data_ptr(), status.data_ptr(), int(max_in_size), self._stream())
        self._check(rc, "rans4x8 peek_dev")

    def uncompress_packed_4x8(self, d_in, in_off, in_size, d_out, out_off, out_size, status, max_in_size, max_out_size,
                              out_capacity=None):
        """rans4x8_hip_uncompress_packed_dev: every block decoded to d_out[out_off[i]:out_off[i + 1]], the sizes taken from
        the streams.  in_off may have n or n + 1 entries (compress_packed_4x8's out_off goes straight in); the block
        count is in_size's."""
        t = self.torch
        n = in_size.numel()
        assert d_in.dtype == t.uint8 and d_out.dtype == t.uint8
        assert in_off.dtype == t.int64 and in_off.numel() >= n and in_size.dtype == t.int32
        assert out_off.dtype == t.int64 and out_off.numel() == n + 1
        assert out_size.dtype == t.int32 and status.dtype == t.int32
        cap = d_out.numel() if out_capacity is None else int(out_capacity)
        assert cap <= d_out.numel()
        rc = self.L.rans4x8_hip_uncompress_packed_dev(
            self.ctx.h, n, d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr(), cap, out_off.data_ptr(), out_size.data_ptr(), status.data_ptr(),
            int(max_in_size), int(max_out_size), self._stream())
        self._check(rc, "rans4x8 uncompress_packed_dev")

    def compress_4x8(self, d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status, order, max_in_size, d_order=None):
        """rans4x8_hip_compress_dev: the slot call (out_off: n entries, read; out_cap: int32, what each slot holds)."""
        t = self.torch
        n = in_off.numel()
        self._slot_args(d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status)
        assert out_off.numel() == n and in_size.numel() == n and out_cap.numel() == n
        assert d_order is None or (d_order.dtype == t.int32 and d_order.numel() == n)
        rc = self.L.rans4x8_hip_compress_dev(
            self.ctx.h, in_off.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(), out_size.data_ptr(), status.data_ptr(), int(order),
            d_order.data_ptr() if d_order is not None else None, int(max_in_size), self._stream())
        self._check(rc, "rans4x8 compress_dev")

    def uncompress_4x8(self, d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status):
        """rans4x8_hip_uncompress_dev: the slot call (in_off may have more than n entries; the block count is in_size's)."""
        n = in_size.numel()
        self._slot_args(d_in, in_off, in_size, d_out, out_off, out_cap, out_size, status)
        assert in_off.numel() >= n and out_off.numel() == n and out_cap.numel() == n
        rc = self.L.rans4x8_hip_uncompress_dev(
            self.ctx.h, in_size.numel(), d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(),
            d_out.data_ptr(), out_off.data_ptr(), out_cap.data_ptr(), out_size.data_ptr(), status.data_ptr(), self._stream())
        self._check(rc, "rans4x8 uncompress_dev")
