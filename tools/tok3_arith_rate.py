#!/usr/bin/env python3
"""What the arith flavour of the tok3 name calls (use_arith = 1, rans4x16_hip_set_tok3_arith) costs beside the rANS
flavour, on the same name blocks, in one process and in alternating passes:

  rans4x16_hip_tok3_encode_names_dev / _decode_names_dev       device-resident, device events
  rans4x16_hip_tok3_encode_names_batch / _decode_names_batch   host buffers in and out, the host's clock around the C call

    python tools/tok3_arith_rate.py [--blocks 512] [--level 9] [--passes 12] [--warmup 3] [--out FILE]

The blocks are those of tools/names_host_rate.py (the names files of tests/golden/names, cycled in the order of the 55
containers of tests/golden/tok3).  Before anything is timed the results are checked: every container decodes to its
names in its own flavour, the host and the device-resident containers are the same bytes, and the first blocks equal the
reference's containers of that level where those are byte-exact (tests/tok3_arith_model.py BYTE_EXACT).  Medians with the
fastest and slowest pass; the slowdown is arith over rANS.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DECODE, ENCODE = 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=512)
    ap.add_argument("--level", type=int, default=9)
    ap.add_argument("--passes", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import tok3_model as M
    import tok3_names_model as N
    import htscodecs_amd as H
    from htscodecs_amd import codec
    if not torch.cuda.is_available():
        sys.exit("tok3_arith_rate: no GPU (there is no CPU path to time)")
    dc = H.DeviceCodec(0)
    L, ctx, dev = dc.L, dc.ctx, dc.dev
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)

    fx = M.fixtures()
    files = N.names_files()
    nblk = args.blocks
    keys = [fx[b % len(fx)][0].split(".")[0] for b in range(nblk)]
    blocks = [files[k] for k in keys]
    methods = codec.tok3_level_methods(args.level)
    in_bytes = sum(len(b) for b in blocks)
    want_names = [b.replace(b"\n", b"\0") for b in blocks]

    def host_args(items):
        srcs = [np.frombuffer(b, dtype=np.uint8) for b in items]
        n = len(items)
        return (srcs, (C.c_void_p * n)(*[s.ctypes.data for s in srcs]), (C.c_uint * n)(*[len(s) for s in srcs]),
                (C.c_void_p * n)(), (C.c_uint * n)(), (C.c_int * n)())

    def host_run(a, encode, arith, keep=False):
        srcs, in_p, in_sz, out_p, out_sz, status = a
        n = len(srcs)
        for i in range(n):
            out_p[i] = None
        meth = (C.c_int * len(methods))(*methods)
        dc.set_tok3_arith((ENCODE if encode else DECODE) if arith else 0)
        t0 = time.perf_counter()
        if encode:
            rc = L.rans4x16_hip_tok3_encode_names_batch(ctx.h, n, in_p, in_sz, out_p, out_sz, len(methods), meth, None, None, status)
        else:
            rc = L.rans4x16_hip_tok3_decode_names_batch(ctx.h, n, in_p, in_sz, out_p, out_sz, None, status)
        ms = (time.perf_counter() - t0) * 1e3
        dc.set_tok3_arith(0)
        assert rc == 0, (rc, ctx.error())
        res = [C.string_at(out_p[i], out_sz[i]) for i in range(n)] if keep else None
        for i in range(n):
            codec._free(out_p[i])
        return ms, res

    # ---- both flavours' containers, checked before anything is timed
    enc_args = host_args(blocks)
    containers, dec_args = {}, {}
    for arith in (0, 1):
        _, containers[arith] = host_run(enc_args, True, arith, keep=True)
        assert all(c[8] == arith for c in containers[arith])
        dec_args[arith] = host_args(containers[arith])
        _, names = host_run(dec_args[arith], False, arith, keep=True)
        assert names == want_names, arith
    by = {os.path.basename(p): open(p, "rb").read() for p in
          [os.path.join(M.GOLDEN, f) for f in os.listdir(M.GOLDEN) if f.endswith(".names.%d" % (10 + args.level))]}
    same = 0
    if args.level in (7, 9):
        for b in range(min(nblk, len(fx))):
            assert containers[1][b] == by["%s.names.%d" % (keys[b], 10 + args.level)], keys[b]
            same += 1

    # ---- the device-resident one-call forms on the same blocks
    maxc, max_names, max_name_len, max_tokens = 64, 1000, 256, 32
    max_in = max(len(b) for b in blocks)
    d_in = t(np.frombuffer(b"".join(blocks) + b"\0" * 64, dtype=np.uint8).copy())
    in_off = t(np.cumsum([0] + [len(b) for b in blocks[:-1]]).astype(np.int64))
    in_size = t(np.array([len(b) for b in blocks], dtype=np.int32))
    e_out = torch.empty(in_bytes + 1024 * nblk, dtype=torch.uint8, device=dev)
    e_off, e_sz, e_st = i64(nblk + 1), i32(nblk), i32(nblk)
    n_out = torch.empty(in_bytes + 64, dtype=torch.uint8, device=dev)
    n_off, n_sz, n_nn, n_st = i64(nblk + 1), i32(nblk), i32(nblk), i32(nblk)
    dec_in = {}
    max_col = 0
    for arith in (0, 1):
        cs = containers[arith]
        scans = [codec.tok3_scan_any(c)[1] for c in cs]
        max_col = max(max_col, max(s["largest_col"] for s in scans))
        dec_in[arith] = (t(np.frombuffer(b"".join(cs) + b"\0" * 64, dtype=np.uint8).copy()),
                         t(np.cumsum([0] + [len(c) for c in cs[:-1]]).astype(np.int64)), t(np.array([len(c) for c in cs], dtype=np.int32)),
                         max(s["ndesc"] for s in scans), max(len(c) for c in cs), max(s["nreads"] for s in scans),
                         sum(s["total_col_size"] for s in scans))
    assert L.rans4x16_hip_set_dev_stripe_planes(ctx.h, 4, max_col) == 0

    def dev_encode(arith):
        dc.set_tok3_arith(ENCODE if arith else 0)
        dc.tok3_encode_names(d_in, in_off, in_size, e_out, e_off, e_sz, e_st, methods, max_in, max_names, max_name_len, maxc,
                             max_tokens=max_tokens, total_in_size=in_bytes)
        dc.set_tok3_arith(0)

    def dev_decode(arith):
        c_in, c_off, c_size, ndesc, c_max, nreads, total = dec_in[arith]
        dc.set_tok3_arith(DECODE if arith else 0)
        dc.tok3_decode_names(c_in, c_off, c_size, n_out, n_off, n_sz, n_nn, n_st, ndesc, c_max, max_col, nreads, 128, total_col_size=total)
        dc.set_tok3_arith(0)

    for arith in (0, 1):
        dev_encode(arith)
        torch.cuda.synchronize()
        assert (e_st == 0).all()
        off = e_off.cpu().numpy()
        got = e_out[:int(off[-1])].cpu().numpy()
        assert [got[off[b]:off[b + 1]].tobytes() for b in range(nblk)] == containers[arith], arith
        dev_decode(arith)
        torch.cuda.synchronize()
        assert (n_st == 0).all()
        off = n_off.cpu().numpy()
        got = n_out[:int(off[-1])].cpu().numpy()
        assert [got[off[b]:off[b + 1]].tobytes() for b in range(nblk)] == want_names, arith

    flavour = ("rans", "arith")
    ms = {"%s_%s_%s" % (d, w, f): [] for d in ("encode", "decode") for w in ("dev", "host") for f in flavour}
    for p in range(args.warmup + args.passes):
        rec = p >= args.warmup
        for arith in (0, 1):
            for d, fn in (("encode", dev_encode), ("decode", dev_decode)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(arith)
                b.record()
                torch.cuda.synchronize()
                if rec:
                    ms["%s_dev_%s" % (d, flavour[arith])].append(a.elapsed_time(b))
            for d, a, enc in (("encode", enc_args, True), ("decode", dec_args[arith], False)):
                v, _ = host_run(a, enc, arith)
                if rec:
                    ms["%s_host_%s" % (d, flavour[arith])].append(v)
    res = {"blocks": nblk, "name_bytes": in_bytes, "level": args.level, "methods": methods, "passes": args.passes, "warmup": args.warmup,
           "container_bytes": {flavour[a]: sum(len(c) for c in containers[a]) for a in (0, 1)}, "reference_containers_matched": same}
    for k, v in ms.items():
        med = statistics.median(v)
        res[k + "_ms"] = {"median": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4), "MB_per_s": round(in_bytes / med / 1e3, 1)}
    for d in ("encode", "decode"):
        for w in ("dev", "host"):
            res["%s_%s_arith_over_rans" % (d, w)] = round(res["%s_%s_arith_ms" % (d, w)]["median"] / res["%s_%s_rans_ms" % (d, w)]["median"], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
