#!/usr/bin/env python3
"""What tok3 name encoding costs beside the column packing it feeds (include/rans4x16_hip.h parts 2c and 2e):

  rans4x16_hip_tok3_tokenise_dev       read names -> token columns (the stage alone)
  rans4x16_hip_tok3_pack_dev           the same columns -> containers (the existing call, n read back once beforehand)
  rans4x16_hip_tok3_encode_names_dev   read names -> containers, one call

    python tools/tok3_enc_rate.py [--blocks 512] [--level 7] [--passes 12] [--warmup 3] [--slots 0] [--out FILE]

The blocks cycle through the names files of tests/golden/names in the order of the 55 containers of tests/golden/tok3
(the batch of tools/tok3_names_rate.py).  All three run in one process, alternating, timed with device events; medians
with the fastest and slowest pass beside them.  Before anything is timed the containers of the one call are compared
with those of the two-call route and with the reference-made fixtures of that level.  Prints one JSON line."""
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
    ap.add_argument("--level", type=int, default=7)
    ap.add_argument("--passes", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slots", type=int, default=0, help="search_slots (1: the exact search alone)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import tok3_model as M
    import tok3_names_model as N
    import htscodecs_amd as H
    if not torch.cuda.is_available():
        sys.exit("tok3_enc_rate: no GPU (there is no CPU path to time)")
    dc = H.DeviceCodec(0)
    dev = dc.dev
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)

    fx = M.fixtures()
    files = N.names_files()
    nblk = args.blocks
    keys = [fx[b % len(fx)][0].split(".")[0] for b in range(nblk)]
    blocks = [files[k] for k in keys]
    methods = M.LISTS[args.level]
    maxc, max_names, max_name_len, max_tokens = 64, 1000, 256, 32
    max_in = max(len(b) for b in blocks)
    in_bytes = sum(len(b) for b in blocks)
    d_in = t(np.frombuffer(b"".join(blocks) + b"\0" * 64, dtype=np.uint8).copy())
    in_off = t(np.cumsum([0] + [len(b) for b in blocks[:-1]]).astype(np.int64))
    in_size = t(np.array([len(b) for b in blocks], dtype=np.int32))

    free0 = torch.cuda.mem_get_info()[0]
    cols = torch.empty(6 * in_bytes + 64, dtype=torch.uint8, device=dev)
    c_off, c_sz, c_st, c_first, c_ls, c_nr = i64(nblk + 1), i32(nblk), i32(nblk), i32(nblk + 1), i32(nblk), i32(nblk)
    c_id, c_coff, c_csz = i32(nblk * maxc), i64(nblk * maxc), i32(nblk * maxc)
    out = [torch.empty(in_bytes + 1024 * nblk, dtype=torch.uint8, device=dev) for _ in range(2)]
    o_off, o_sz, o_st = [i64(nblk + 1) for _ in range(2)], [i32(nblk) for _ in range(2)], [i32(nblk) for _ in range(2)]

    tokenise = lambda: dc.tok3_tokenise(d_in, in_off, in_size, cols, c_off, c_sz, c_st, c_first, c_id, c_coff, c_csz, c_ls, c_nr,
                                        max_in, max_names, max_name_len, maxc, max_tokens=max_tokens, total_in_size=in_bytes,
                                        search_slots=args.slots)
    tokenise()
    torch.cuda.synchronize()
    assert (c_st == 0).all()
    n = int(c_first[nblk])
    col_bytes = int(c_off[nblk])
    max_col = int(c_csz[:n].max())
    calls = {
        "tok3_tokenise": tokenise,
        "tok3_pack": lambda: dc.tok3_pack(c_first, cols, c_coff[:n], c_csz[:n], c_id[:n], c_ls, c_nr, out[0], o_off[0], o_sz[0], o_st[0],
                                          methods, max_col, total_col_size=col_bytes),
        "tok3_encode_names": lambda: dc.tok3_encode_names(d_in, in_off, in_size, out[1], o_off[1], o_sz[1], o_st[1], methods, max_in,
                                                          max_names, max_name_len, maxc, max_tokens=max_tokens, max_col_size=max_col,
                                                          total_in_size=in_bytes, search_slots=args.slots),
    }
    # once, checked, before anything is timed
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    off = [o.cpu().numpy() for o in o_off]
    assert (o_st[0] == 0).all() and (o_st[1] == 0).all() and np.array_equal(off[0], off[1])
    got = [o[:int(off[0][-1])].cpu().numpy() for o in out]
    assert np.array_equal(got[0], got[1])
    by = dict(fx)
    same = 0
    for b in range(min(nblk, len(fx))):
        name = "%s.names.%d" % (keys[b], args.level)
        if name not in M.EXCEPTIONS:
            assert got[1][off[1][b]:off[1][b + 1]].tobytes() == by[name], name
            same += 1

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
    res = {"blocks": nblk, "names": 1000 * nblk, "name_bytes": in_bytes, "columns": n, "column_bytes": col_bytes,
           "container_bytes": int(off[0][-1]), "level": args.level, "methods": methods, "max_columns": maxc, "max_names": max_names,
           "max_tokens": max_tokens, "search_slots": args.slots, "passes": args.passes, "fixtures_matched": same,
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
