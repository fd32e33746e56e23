#!/usr/bin/env python3
"""What tok3 name decoding costs beside the column decode it follows (include/rans4x16_hip.h parts 2c and 2d):

  rans4x16_hip_tok3_decode_names_dev   containers -> read names, one call
  rans4x16_hip_tok3_unpack_dev         containers -> token columns (the first half, unchanged by part 2d)
  rans4x16_hip_tok3_names_dev          token columns -> read names (the second half)
  a device-to-host copy of the column bytes into pinned memory: what a caller pays before a CPU tokeniser can start

    python tools/tok3_names_rate.py [--blocks 512] [--passes 12] [--warmup 3] [--out FILE]

The blocks cycle through the 55 containers of tests/golden/tok3.  All four run in one process, alternating, timed with
device events; medians with the fastest and slowest pass beside them.  The names are compared with tests/golden/names
before anything is timed.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=512)
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
        sys.exit("tok3_names_rate: no GPU (there is no CPU path to time)")
    dc = H.DeviceCodec(0)
    dev = dc.dev
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)

    fx = M.fixtures()
    files = N.names_files()
    info = [codec.tok3_scan(b)[1] for _, b in fx]
    maxc, max_col, max_names, max_tokens = 64, max(i["largest_col"] for i in info), 1000, 32
    assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, 4, max_col) == 0
    nblk = args.blocks
    pick = [b % len(fx) for b in range(nblk)]
    conts = [fx[f][1] for f in pick]
    want = [files[fx[f][0].split(".")[0]].replace(b"\n", b"\0") for f in pick]
    col_bytes = sum(info[f]["total_col_size"] for f in pick)
    name_bytes = sum(len(w) for w in want)
    d_in = t(np.frombuffer(b"".join(conts) + b"\0" * 64, dtype=np.uint8).copy())
    in_off = t(np.cumsum([0] + [len(c) for c in conts[:-1]]).astype(np.int64))
    in_size = t(np.array([len(c) for c in conts], dtype=np.int32))
    max_in = max(len(c) for c in conts)

    free0 = torch.cuda.mem_get_info()[0]
    cols = torch.empty(col_bytes + 64, dtype=torch.uint8, device=dev)
    u_off, u_sz, u_st, u_nc, u_ls, u_nr = i64(nblk + 1), i32(nblk), i32(nblk), i32(nblk), i32(nblk), i32(nblk)
    u_id, u_coff, u_csz = i32(nblk * maxc), i64(nblk * maxc), i32(nblk * maxc)
    names = [torch.empty(name_bytes + 64, dtype=torch.uint8, device=dev) for _ in range(2)]
    n_off, n_sz, n_nn, n_st = [i64(nblk + 1) for _ in range(2)], [i32(nblk) for _ in range(2)], [i32(nblk) for _ in range(2)], [i32(nblk) for _ in range(2)]
    starts = i32(nblk * max_names)
    host = torch.empty(col_bytes, dtype=torch.uint8).pin_memory()

    calls = {
        "tok3_decode_names": lambda: dc.tok3_decode_names(d_in, in_off, in_size, names[0], n_off[0], n_sz[0], n_nn[0], n_st[0], maxc, max_in,
                                                          max_col, max_names, max_tokens, total_col_size=col_bytes, name_start=starts,
                                                          out_capacity=name_bytes),
        "tok3_unpack": lambda: dc.tok3_unpack(d_in, in_off, in_size, cols, u_off, u_sz, u_st, u_nc, u_ls, u_nr, u_id, u_coff, u_csz,
                                              maxc, max_in, max_col, out_capacity=col_bytes),
        "tok3_names": lambda: dc.tok3_names(cols[:col_bytes], u_id, u_coff, u_csz, u_nc, u_ls, u_nr, names[1], n_off[1], n_sz[1], n_nn[1], n_st[1],
                                            maxc, max_names, max_tokens, blk_status=u_st, name_start=starts, out_capacity=name_bytes),
        "columns_to_host": lambda: host.copy_(cols[:col_bytes], non_blocking=True),
    }
    # once, checked, before anything is timed
    for name in ("tok3_decode_names", "tok3_unpack", "tok3_names"):
        calls[name]()
    torch.cuda.synchronize()
    expect = b"".join(want)
    for k in range(2):
        assert (n_st[k] == 0).all() and int(n_nn[k].sum()) == 1000 * nblk, k
        assert names[k][:name_bytes].cpu().numpy().tobytes() == expect, k

    ms = {k: [] for k in calls}
    for p in range(args.warmup + args.passes):
        for name, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if p >= args.warmup:
                ms[name].append(a.elapsed_time(b))
    res = {"blocks": nblk, "names": 1000 * nblk, "container_bytes": sum(len(c) for c in conts), "column_bytes": col_bytes,
           "name_bytes": name_bytes, "max_columns": maxc, "max_names": max_names, "max_tokens": max_tokens, "passes": args.passes,
           "workspace_bytes": dc.workspace_bytes(), "device_bytes_taken": free0 - torch.cuda.mem_get_info()[0]}
    for k, v in ms.items():
        res[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
