"""Hostile X_STRIPE input (rANS_static4x16pr.c:1360-1433): the header of a stripe stream - stored length, plane count N,
N plane lengths - is read straight from the stream, and k_stripe_dec_prepare (r4x16_stripe.hip) and the host entry points
(r4x16_host.hip) lay out their work from it.  A fixed corpus of oracle-made stripe streams with every header field edited
in turn (the edits are named, and come first), plus random damage in the modes of tests/soak/fuzz_damaged_gpu.py, goes
through the oracle - plain and under ASan/UBSan - and through three routes of the library:

    the host batch call with the device stripe kernels (host_stripe_dev 1), the same with the host-side orchestration
    (host_stripe_dev 0), and rans4x16_hip_uncompress_dev after rans4x16_hip_set_dev_stripe_planes(7, 1 << 16).

Contract per case: what the oracle rejects the library rejects (status != 0, size 0); what both accept is byte-identical;
the library may refuse what the oracle accepts only with UNSUPPORTED where the stream's own bytes say why (more planes
than reserved, a stored size above the reserved plane buffer, a plane that is itself a stripe stream), with CONTEXT / RLE
(7, 8: the documented stricter cases) where that is the verdict on one of the planes, or with CAPACITY where the stored
size is not the capacity handed in.  Nothing is written outside the callers' buffers (test_gpu_confinement.py's layout),
and the context decodes valid streams afterwards."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import datagen
from test_gpu_confinement import Layout, _Guarded, _host_call

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BASE_ORDERS = [8, 9, 0x48, 0xc9, (2 << 8) | 9, (3 << 8) | 0xc9, (7 << 8) | 8]
DEV_PLANES, DEV_SIZE = 7, 1 << 16
CAP_LIMIT = 1 << 16


def put_varint(v):
    groups = [v & 0x7f]
    v >>= 7
    while v:
        groups.append((v & 0x7f) | 0x80)
        v >>= 7
    return bytes(reversed(groups))


def get_varint(b, pos, end):
    """(value, bytes used) the way the library reads one (varint.h:131-160, bounded by `end`)."""
    v, used = 0, 0
    if pos >= end:
        return 0, 0
    while True:
        ch = b[pos + used]
        used += 1
        v = ((v << 7) | (ch & 0x7f)) & 0xffffffff
        if not (ch & 0x80 and pos + used < end):
            return v, used


def parse(b):
    """The stripe header as :1360-1400 reads it: None if the stream is no stripe stream or ends inside the fixed part, else a
    dict - ulen, N, the spans of the fields, and `planes`: [(offset, length field)] when the plane list passes the checks
    of :1389 / :1398 (else None)."""
    n = len(b)
    if n == 0 or not b[0] & 8:
        return None
    ulen, used = get_varint(b, 1, n)
    hdr = 1 + used
    if hdr >= n:
        return None
    h = {"ulen": ulen, "ulen_span": (1, hdr), "N_pos": hdr, "N": b[hdr], "planes": None, "cl_spans": []}
    hdr += 1
    cl, ctot = [], 0
    for j in range(h["N"]):
        v, used = get_varint(b, hdr, n)
        h["cl_spans"].append((hdr, hdr + used))
        hdr += used
        cl.append(v)
        ctot += v
        if hdr > n or v > n or v < 1:
            return h
    if hdr + ctot > n:
        return h
    h["hdr"], h["used"] = hdr, hdr + ctot
    h["planes"] = [(hdr + sum(cl[:j]), cl[j]) for j in range(h["N"])]
    return h


def base_streams(oracle):
    """About forty (input, stripe stream) pairs: every stripe flag set, inputs of 24 .. 20,000 bytes."""
    out = []
    sizes = [24, 25, 27, 30, 100, 101, 254, 999, 1000, 1003, 4096, 4099, 9998, 20000]
    for k in range(42):
        n = sizes[(5 * k) % len(sizes)]
        order = BASE_ORDERS[k % len(BASE_ORDERS)]
        kind = k % 4
        if kind == 0: d = datagen.tile(("q4", "q8", "q40+dir", "qvar")[(k // 4) % 4], n, k)
        elif kind == 1: d = np.random.RandomState(k).randint(0, 70000, n // 4 + 1).astype("<u4").tobytes()[:n]
        elif kind == 2: d = datagen.runs(n, 5, 9, k + 1, 40)
        else: d = datagen.rand(n, k + 1, 1 + (7 * k) % 40, 60)
        d = bytes(np.ascontiguousarray(d).tobytes()) if not isinstance(d, bytes) else d
        out.append((d, oracle.compress(d, order), order))
    return out


def targeted(d, s, order, oracle, k):
    """[(name, mutant)] of one base stream: every header field in turn."""
    h = parse(s)
    assert h and h["planes"], "the oracle's own stream does not parse"
    N, ulen, npos = h["N"], h["ulen"], h["N_pos"]
    (u0, u1), spans, planes = h["ulen_span"], h["cl_spans"], h["planes"]
    out = []
    setb = lambda pos, v: s[:pos] + bytes([v]) + s[pos + 1:]
    span = lambda a, b, new: s[:a] + new + s[b:]
    for name, v in (("N=0", 0), ("N=1", 1), ("N-1", N - 1), ("N+1", N + 1), ("N=255", 255)):
        out.append((name, setb(npos, v)))
    for name, v in (("len=0", 0), ("len=N-1", N - 1), ("len-1", ulen - 1), ("len+1", ulen + 1), ("len=2^31-2", (1 << 31) - 2)):
        out.append((name, span(u0, u1, put_varint(v))))
    j = k % N
    a, b = spans[j]
    for name, new in (("plane=0", b"\x00"), ("plane=in_size", put_varint(len(s))), ("plane=in_size+1", put_varint(len(s) + 1)),
                      ("plane=2^32-1", b"\x8f\xff\xff\xff\x7f")):
        out.append((name, span(a, b, new)))
    a, b = spans[-1]
    out.append(("sum+1", span(a, b, put_varint(planes[-1][1] + 1))))
    out.append(("cut-in-len", s[:u1 - 1] if u1 - u0 > 1 else s[:1]))
    out.append(("cut-in-list", s[:spans[N // 2][0] + (1 if N // 2 else 0)] if N > 1 else s[:spans[0][0]]))
    for j, (off, ln) in enumerate(planes):
        out.append(("cut-in-plane", s[:off + ln // 2]))
    for j, (off, ln) in enumerate(planes):                 # damage below the header: the planes' own verdicts
        p = off + ln - 1 - (k + j) % max(ln // 2, 1)
        out.append(("plane-byte", setb(p, s[p] ^ (1 << ((k + j) % 8)))))
    out.append(("slack", s + bytes([k & 0xff] * (1 + k % 9))))
    out.append(("nested", setb(planes[0][0], s[planes[0][0]] | 8)))
    if len(d) // N > 20:                                   # ... and one the oracle decodes: plane 0 as a stripe stream of its own
        inner = oracle.compress(d[0::N], 9)
        cls = b"".join(put_varint(len(inner) if j == 0 else ln) for j, (_, ln) in enumerate(planes))
        out.append(("nested-valid", s[:spans[0][0]] + cls + inner + s[planes[1][0]:]))
    plain = oracle.compress(d, order & 0xf7)
    out.append(("flag-on-ordinary", bytes([plain[0] | 8]) + plain[1:]))
    return out


def mutate(rs, comp, others):
    """The modes of tests/soak/fuzz_damaged_gpu.py; the stripe flag stays (ordinary streams have their own tests)."""
    bad = bytearray(comp)
    mode = int(rs.randint(0, 7))
    if mode == 0:                                   # one bit anywhere
        p = int(rs.randint(0, len(bad))); bad[p] ^= 1 << int(rs.randint(0, 8))
    elif mode == 1:                                 # truncate
        bad = bad[:int(rs.randint(1, len(bad) + 1))]
    elif mode == 2:                                 # smash a byte in the header / table region
        p = int(rs.randint(0, min(len(bad), 64))); bad[p] = int(rs.randint(0, 256))
    elif mode == 3:                                 # several byte smashes anywhere
        for _ in range(int(rs.randint(1, 6))):
            p = int(rs.randint(0, len(bad))); bad[p] = int(rs.randint(0, 256))
    elif mode == 4:                                 # splice the tail of another stream
        o = others[int(rs.randint(0, len(others)))]
        cut = int(rs.randint(1, len(bad) + 1))
        bad = bad[:cut] + bytearray(o[int(rs.randint(0, len(o))):])
    elif mode == 5:                                 # extreme values where sizes and counts live
        p = int(rs.randint(0, min(len(bad), 24))); bad[p] = int(rs.choice([0, 0x7f, 0x80, 0xff]))
    else:                                           # insert or delete a few bytes
        p = int(rs.randint(0, len(bad)))
        if rs.randint(0, 2): del bad[p:p + int(rs.randint(1, 4))]
        else: bad[p:p] = bytes(rs.randint(0, 256, int(rs.randint(1, 4))).astype(np.uint8))
    if not len(bad):
        bad = bytearray(b"\x00")
    bad[0] |= 8
    return bytes(bad)


_CORPUS = None


def corpus(oracle):
    """[(edit name, stream, capacity, the oracle's bytes or None)], the targeted edits first.  The capacity is the original
    length for every other case and the stream's own size field, bounded to 1 << 16, for the rest."""
    global _CORPUS
    if _CORPUS is None:
        bases = base_streams(oracle)
        cases = []
        for k, (d, s, order) in enumerate(bases):
            cases += [(name, m, len(d)) for name, m in targeted(d, s, order, oracle, k)]
        rs = np.random.RandomState(2026)
        comps = [s for _, s, _ in bases]
        for d, s, _ in bases:
            cases += [("random", mutate(rs, s, comps), len(d)) for _ in range(5)]
        out = []
        for i, (name, m, n) in enumerate(cases):
            cap = n if i % 2 == 0 else min(get_varint(m, 1, len(m))[0], CAP_LIMIT)
            out.append((name, m, cap, oracle.uncompress(m, capacity=cap, out_size_hint=cap)))
        _CORPUS = out
    return _CORPUS


EDITS = ["N=0", "N=1", "N-1", "N+1", "N=255", "len=0", "len=N-1", "len-1", "len+1", "len=2^31-2", "plane=0", "plane=in_size",
         "plane=in_size+1", "plane=2^32-1", "sum+1", "cut-in-len", "cut-in-list", "cut-in-plane", "plane-byte", "slack", "nested",
         "nested-valid", "flag-on-ordinary", "random"]


# ---- CPU --------------------------------------------------------------------------------------------------------
def test_corpus_holds_what_it_claims(oracle):
    cases = corpus(oracle)
    assert {name for name, _, _, _ in cases} == set(EDITS)
    assert all(m[0] & 8 for _, m, _, _ in cases) and max(len(m) for _, m, _, _ in cases) < 70000
    acc = sum(r is not None for _, _, _, r in cases)
    by = {}
    for name, _, _, r in cases:
        a = by.setdefault(name, [0, 0])
        a[r is None] += 1
    print("cases", len(cases), "oracle accepts", acc, "rejects", len(cases) - acc, by)
    assert 4 * acc >= len(cases) and 4 * (len(cases) - acc) >= len(cases), (acc, len(cases))
    for (d, s, _) in base_streams(oracle):
        assert oracle.uncompress(s, capacity=len(d), out_size_hint=len(d)) == d
    # the device-side predicates have something to bite on
    assert sum(1 for _, m, _, _ in cases if (parse(m) or {}).get("N", 0) > DEV_PLANES) >= 40
    assert sum(1 for _, m, _, _ in cases if (parse(m) or {}).get("ulen", 0) > DEV_SIZE) >= 40
    assert sum(1 for _, m, _, _ in cases if _nested(m)) >= 40
    assert sum(1 for name, m, _, r in cases if name == "nested-valid" and _nested(m) and r is not None) >= 20


CHILD = r'''
import ctypes as C, pickle, sys
lib = C.CDLL(sys.argv[1])
libc = C.CDLL(None)
libc.malloc.restype = C.c_void_p; libc.malloc.argtypes = [C.c_size_t]; libc.free.argtypes = [C.c_void_p]
fn = lib.orc_rans_uncompress_to_4x16
fn.restype = C.c_void_p; fn.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.POINTER(C.c_uint)]
cases = pickle.load(open(sys.argv[2], "rb"))
verdicts = []
for m, cap in cases:
    src = libc.malloc(len(m) + 32)                # slack: the table readers look ahead by design
    C.memmove(src, m + bytes(32), len(m) + 32)
    out = libc.malloc(max(cap, 1))                # exactly the capacity: a write past it is a finding
    n = C.c_uint(cap)
    r = fn(src, len(m), out, C.byref(n))
    verdicts.append(C.string_at(out, n.value) if r else None)
    libc.free(src); libc.free(out)
pickle.dump(verdicts, open(sys.argv[3], "wb"))
print("sanitized cases:", len(cases))
'''


def test_oracle_verdicts_hold_under_asan_ubsan(oracle, tmp_path):
    """The expected outcomes do not come from undefined behaviour in the checker: the sanitizer build of the oracle
    (test_oracle_sanitized.py) gives the same verdict and the same bytes on every case, and reports nothing."""
    cases = corpus(oracle)
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "liboracle4x16_asan.so"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build not available: " + r.stdout[-300:])
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], stdout=subprocess.PIPE, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("libasan.so not found")
    with open(tmp_path / "cases", "wb") as f:
        pickle.dump([(m, cap) for _, m, cap, _ in cases], f)
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:allocator_may_return_null=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "oracle", "liboracle4x16_asan.so"),
                        str(tmp_path / "cases"), str(tmp_path / "verdicts")],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "sanitized cases: %d" % len(cases) in r.stdout
    with open(tmp_path / "verdicts", "rb") as f:
        verdicts = pickle.load(f)
    diff = [(i, cases[i][0]) for i in range(len(cases)) if verdicts[i] != cases[i][3]]
    assert not diff, diff[:10]


# ---- the contract -----------------------------------------------------------------------------------------------
def _nested(m):
    h = parse(m)
    return bool(h and h["planes"] and any(m[off] & 8 for off, _ in h["planes"]))


def _sub_streams(m):
    """[(bytes, capacity)] of the planes as the library hands them on: each may read to the end of the block (:1419)."""
    h = parse(m)
    N, ulen = h["N"], h["ulen"]
    return [(m[off:h["used"]], ulen // N + (ulen % N > j)) for j, (off, _) in enumerate(h["planes"])]


def judge(H, cases, st, osz, got, planes_reserved, size_reserved):
    """(violations, number of cases the library refused although the oracle accepts them - with an allowed status)."""
    bad, stricter, ask = [], 0, []
    for i, (name, m, cap, ref) in enumerate(cases):
        where = (i, name, "flags %#x len %d cap %d" % (m[0], len(m), cap), "status %d size %d" % (st[i], osz[i]))
        if ref is None:
            if st[i] == 0 or osz[i] != 0:
                bad.append(("ACCEPTED what the oracle rejects",) + where)
        elif st[i] == 0:
            if got[i] != ref:
                bad.append(("DIFFERENT BYTES",) + where)
        else:
            stricter += 1
            h = parse(m)
            if osz[i] != 0:
                bad.append(("a size with a failure",) + where)
            elif st[i] == 6:
                if not (h and ((planes_reserved is not None and h["N"] > planes_reserved) or
                               (size_reserved is not None and h["ulen"] > size_reserved) or _nested(m))):
                    bad.append(("UNSUPPORTED without a reason in the stream",) + where)
            elif st[i] in (7, 8):
                if h and h["planes"]:
                    ask.append((i, where))
                else:
                    bad.append(("a plane's verdict on a stream without planes",) + where)
            elif st[i] == 1:
                if not (h and h["ulen"] != cap):
                    bad.append(("CAPACITY although the stored size is the capacity",) + where)
            else:
                bad.append(("REJECTED what the oracle accepts",) + where)
    if ask:                                                # 7 / 8 must be the verdict on one of the planes, decoded on its own
        subs, owner = [], []
        for i, where in ask:
            for sub, cap in _sub_streams(cases[i][1]):
                subs.append(sub); owner.append(i)
        _, sst = H.uncompress_batch(subs, [c for i, _ in ask for _, c in _sub_streams(cases[i][1])])
        for i, where in ask:
            mine = [s for s, o in zip(sst, owner) if o == i and s != 0]
            if not mine or mine[0] != st[i]:
                bad.append(("status is not the first failing plane's %r" % (mine[:1],),) + where)
    return bad, stricter


def _valid(oracle):
    return [(d, s) for d, s, _ in base_streams(oracle)][:20]


@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd


def _run_host(H, cases):
    lay = Layout([cap for _, _, cap, _ in cases], [name for name, _, _, _ in cases])
    arena = lay.pattern.copy()
    rc, st, osz = _host_call(H, "rans4x16_hip_uncompress_batch", [m for _, m, _, _ in cases], lay, arena)
    stray = lay.stray_writes(arena)
    assert stray is None, stray
    assert rc == int((st != 0).sum())
    return st, osz, lay.take(arena, osz)


def _run_dev(H, dc, cases):
    G = _Guarded(dc.dev, [m for _, m, _, _ in cases], [cap for _, _, cap, _ in cases], [name for name, _, _, _ in cases])
    dc.uncompress(*G.args(), G.max_in, max(G.max_cap, 1))
    return G.results("hostile stripe streams, device-resident")


ROUTES = ["host-stripe-dev", "host-stripe-host", "device-resident"]


def _run(H, oracle, opts, route, cases):
    """(violations, stricter count) of `cases` on one route; valid streams must decode on the same context afterwards."""
    if route == "device-resident":
        dc = H.DeviceCodec(0)
        assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, DEV_PLANES, DEV_SIZE) == 0
        try:
            st, osz, got = _run_dev(H, dc, cases)
            res = judge(H, cases, st, osz, got, DEV_PLANES, DEV_SIZE)
            good = [("valid", s, len(d), d) for d, s in _valid(oracle)]
            st, osz, got = _run_dev(H, dc, good)
        finally:
            assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, 0, 0) == 0
    else:
        opts.set("host_stripe_dev", 1 if route == "host-stripe-dev" else 0)
        st, osz, got = _run_host(H, cases)
        res = judge(H, cases, st, osz, got, None, None)
        good = [("valid", s, len(d), d) for d, s in _valid(oracle)]
        st, osz, got = _run_host(H, good)
    alive = [(i, int(st[i])) for i in range(len(good)) if st[i] != 0 or got[i] != good[i][3]]
    assert not alive, ("valid streams no longer decode", alive)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("edit", EDITS)
@pytest.mark.parametrize("route", ROUTES)
def test_edited_stripe_streams(H, oracle, opts, route, edit):
    cases = [c for c in corpus(oracle) if c[0] == edit]
    bad, stricter = _run(H, oracle, opts, route, cases)
    print(route, edit, "cases", len(cases), "oracle accepts", sum(c[3] is not None for c in cases), "library stricter", stricter)
    assert not bad, bad[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_whole_corpus_in_one_batch_and_the_stricter_share(H, oracle, opts, route):
    """The whole corpus as one batch (damaged neighbours of every kind side by side); at most one case in ten may be
    refused by the library although the oracle accepts it."""
    cases = corpus(oracle)
    bad, stricter = _run(H, oracle, opts, route, cases)
    print(route, "cases", len(cases), "oracle accepts", sum(c[3] is not None for c in cases), "library stricter", stricter)
    assert not bad, bad[:10]
    assert 10 * stricter <= len(cases), (stricter, len(cases))
