#!/usr/bin/env python3
"""What the host-buffer names calls cost beside the device-resident one-call forms (include/rans4x16_hip.h parts 2d to 2f):

  rans4x16_hip_tok3_encode_names_batch / _decode_names_batch   host buffers in and out
  rans4x16_hip_tok3_encode_names_dev / _decode_names_dev       the same blocks, device-resident
  rans4x16_hip_tok3_encode_names / _decode_names               one block through the two drop-in functions

    python tools/names_host_rate.py [--blocks 512] [--level 9] [--passes 12] [--warmup 3] [--out FILE]

The blocks are those of tools/tok3_enc_rate.py (the names files of tests/golden/names, cycled in the order of the 55
containers of tests/golden/tok3).  Host calls synchronise and are timed with the host's clock around the C call (its
ctypes arguments built beforehand); device calls with device events.  All run in one process, alternating; medians with
the fastest and slowest pass.  Before anything is timed the host results are compared with the device-resident ones.
Prints one JSON line."""
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
        sys.exit("names_host_rate: no GPU (there is no CPU path to time)")
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

    # ---- the host calls: arguments once, results freed after every call
    def host_args(items):
        srcs = [np.frombuffer(b, dtype=np.uint8) for b in items]
        n = len(items)
        return (srcs, (C.c_void_p * n)(*[s.ctypes.data for s in srcs]), (C.c_uint * n)(*[len(s) for s in srcs]),
                (C.c_void_p * n)(), (C.c_uint * n)(), (C.c_int * n)())

    def host_run(a, encode, keep=False):
        srcs, in_p, in_sz, out_p, out_sz, status = a
        n = len(srcs)
        for i in range(n):
            out_p[i] = None
        meth = (C.c_int * len(methods))(*methods)
        t0 = time.perf_counter()
        if encode:
            rc = L.rans4x16_hip_tok3_encode_names_batch(ctx.h, n, in_p, in_sz, out_p, out_sz, len(methods), meth, None, None, status)
        else:
            rc = L.rans4x16_hip_tok3_decode_names_batch(ctx.h, n, in_p, in_sz, out_p, out_sz, None, status)
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, (rc, ctx.error())
        res = [C.string_at(out_p[i], out_sz[i]) for i in range(n)] if keep else None
        for i in range(n):
            codec._free(out_p[i])
        return ms, res

    enc_args = host_args(blocks)
    _, containers = host_run(enc_args, True, keep=True)
    dec_args = host_args(containers)
    _, names = host_run(dec_args, False, keep=True)
    assert names == [b.replace(b"\n", b"\0") for b in blocks]
    by = dict(fx)
    same = 0
    for b in range(min(nblk, len(fx))):
        name = "%s.names.%d" % (keys[b], args.level)
        if name in by and name not in M.EXCEPTIONS and M.LISTS.get(args.level) == methods:
            assert containers[b] == by[name], name
            same += 1

    # ---- the device-resident one-call forms on the same blocks
    maxc, max_names, max_name_len, max_tokens = 64, 1000, 256, 32
    max_in = max(len(b) for b in blocks)
    d_in = t(np.frombuffer(b"".join(blocks) + b"\0" * 64, dtype=np.uint8).copy())
    in_off = t(np.cumsum([0] + [len(b) for b in blocks[:-1]]).astype(np.int64))
    in_size = t(np.array([len(b) for b in blocks], dtype=np.int32))
    e_out = torch.empty(in_bytes + 1024 * nblk, dtype=torch.uint8, device=dev)
    e_off, e_sz, e_st = i64(nblk + 1), i32(nblk), i32(nblk)
    scans = [codec.tok3_scan(c)[1] for c in containers]
    c_in = t(np.frombuffer(b"".join(containers) + b"\0" * 64, dtype=np.uint8).copy())
    c_off = t(np.cumsum([0] + [len(c) for c in containers[:-1]]).astype(np.int64))
    c_size = t(np.array([len(c) for c in containers], dtype=np.int32))
    n_out = torch.empty(in_bytes + 64, dtype=torch.uint8, device=dev)
    n_off, n_sz, n_nn, n_st = i64(nblk + 1), i32(nblk), i32(nblk), i32(nblk)
    max_col = max(s["largest_col"] for s in scans)
    assert L.rans4x16_hip_set_dev_stripe_planes(ctx.h, 4, max_col) == 0
    dev_calls = {
        "encode_names_dev": lambda: dc.tok3_encode_names(d_in, in_off, in_size, e_out, e_off, e_sz, e_st, methods, max_in, max_names,
                                                         max_name_len, maxc, max_tokens=max_tokens, total_in_size=in_bytes),
        "decode_names_dev": lambda: dc.tok3_decode_names(c_in, c_off, c_size, n_out, n_off, n_sz, n_nn, n_st, max(s["ndesc"] for s in scans),
                                                         max(len(c) for c in containers), max_col, max(s["nreads"] for s in scans), 128,
                                                         total_col_size=sum(s["total_col_size"] for s in scans)),
    }
    for fn in dev_calls.values():
        fn()
    torch.cuda.synchronize()
    assert (e_st == 0).all() and (n_st == 0).all()
    off = e_off.cpu().numpy()
    got = e_out[:int(off[-1])].cpu().numpy()
    assert [got[off[b]:off[b + 1]].tobytes() for b in range(nblk)] == containers

    # ---- one block through the drop-in functions
    one = blocks[0]
    one_c = containers[0]

    def single_encode():
        t0 = time.perf_counter()
        r = codec.encode_names(one, args.level)
        ms = (time.perf_counter() - t0) * 1e3
        assert r is not None and r[0] == one_c
        return ms

    def single_decode():
        t0 = time.perf_counter()
        r = codec.decode_names(one_c)
        ms = (time.perf_counter() - t0) * 1e3
        assert r == one.replace(b"\n", b"\0")
        return ms

    ms = {k: [] for k in ("encode_names_batch", "decode_names_batch", "encode_names_dev", "decode_names_dev", "encode_names_single",
                          "decode_names_single")}
    for p in range(args.warmup + args.passes):
        rec = p >= args.warmup
        for name, (a, enc) in (("encode_names_batch", (enc_args, True)), ("decode_names_batch", (dec_args, False))):
            v, _ = host_run(a, enc)
            if rec:
                ms[name].append(v)
        for name, fn in dev_calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if rec:
                ms[name].append(a.elapsed_time(b))
        for name, fn in (("encode_names_single", single_encode), ("decode_names_single", single_decode)):
            v = fn()
            if rec:
                ms[name].append(v)
    res = {"blocks": nblk, "name_bytes": in_bytes, "container_bytes": sum(len(c) for c in containers), "level": args.level,
           "methods": methods, "passes": args.passes, "warmup": args.warmup, "fixtures_matched": same,
           "single_block_bytes": len(one)}
    for k, v in ms.items():
        res[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    for d in ("encode", "decode"):
        res[d + "_host_minus_dev_ms"] = round(res[d + "_names_batch_ms"]["median"] - res[d + "_names_dev_ms"]["median"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
