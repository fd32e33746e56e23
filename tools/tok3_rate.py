#!/usr/bin/env python3
"""What the tok3 framing costs on top of the encodes and decodes it is built on (include/rans4x16_hip.h part 2c):

  rans4x16_hip_tok3_pack_dev    against  rans4x16_hip_compress_best_packed_dev  on the same columns
  rans4x16_hip_tok3_unpack_dev  against  rans4x16_hip_uncompress_packed_dev     on the same streams

    python tools/tok3_rate.py [--blocks 512] [--passes 12] [--warmup 3] [--out FILE]

The blocks cycle through the column sets of the containers in tests/golden/tok3 (decoded on the device by the unpack call
itself), method list tokenise_name3.c:1259.  All four calls run in one process, alternating, timed with device events;
medians with the fastest and slowest pass beside them.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NINE = [0, 1, 128, 129, 64, 65, 192, 193, 201]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=512)
    ap.add_argument("--passes", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import tok3_model as M
    import htscodecs_amd as H
    from htscodecs_amd import codec
    if not torch.cuda.is_available():
        sys.exit("tok3_rate: no GPU (there is no CPU path to time)")
    dc = H.DeviceCodec(0)
    dev = dc.dev
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)

    # the fixtures' columns, decoded by the call under test (tests/test_gpu_tok3.py checks it against the oracle)
    fx = [b for _, b in M.fixtures()]
    info = [codec.tok3_scan(b)[1] for b in fx]
    maxc, max_col = 64, max(i["largest_col"] for i in info)
    assert dc.L.rans4x16_hip_set_dev_stripe_planes(dc.ctx.h, 4, max_col) == 0
    nf = len(fx)
    f_in = t(np.frombuffer(b"".join(fx) + b"\0" * 64, dtype=np.uint8))
    f_off = t(np.cumsum([0] + [len(b) for b in fx[:-1]]).astype(np.int64))
    f_size = t(np.array([len(b) for b in fx], dtype=np.int32))
    f_out = torch.empty(sum(i["total_col_size"] for i in info) + 64, dtype=torch.uint8, device=dev)
    o_off, o_sz, o_st, o_nc, o_ls, o_nr = i64(nf + 1), i32(nf), i32(nf), i32(nf), i32(nf), i32(nf)
    c_id, c_off, c_sz = i32(nf * maxc), i64(nf * maxc), i32(nf * maxc)
    dc.tok3_unpack(f_in, f_off, f_size, f_out, o_off, o_sz, o_st, o_nc, o_ls, o_nr, c_id, c_off, c_sz, maxc, max(len(b) for b in fx), max_col)
    torch.cuda.synchronize()
    assert (o_st == 0).all()
    arena = f_out.cpu().numpy()
    ids, offs, szs = c_id.cpu().numpy().reshape(nf, maxc), c_off.cpu().numpy().reshape(nf, maxc), c_sz.cpu().numpy().reshape(nf, maxc)
    ncol, ls, nr = o_nc.cpu().numpy(), o_ls.cpu().numpy(), o_nr.cpu().numpy()

    nblk = args.blocks
    data, col_id, col_size, first, b_ls, b_nr = [], [], [], [0], [], []
    for b in range(nblk):
        f = b % nf
        for c in range(int(ncol[f])):
            if szs[f, c] == 0:
                continue                                        # (a copy of a column that never was: nothing to encode)
            data.append(arena[offs[f, c]:offs[f, c] + szs[f, c]])
            col_id.append(int(ids[f, c]) & 2047)
            col_size.append(int(szs[f, c]))
        first.append(len(col_id))
        b_ls.append(int(ls[f])); b_nr.append(int(nr[f]))
    n, total = len(col_id), int(sum(col_size))
    d_in = t(np.concatenate(data + [np.zeros(64, dtype=np.uint8)]))
    d_coff = t(np.cumsum([0] + col_size[:-1]).astype(np.int64))
    d_csz, d_cid, d_first = t(np.array(col_size, dtype=np.int32)), t(np.array(col_id, dtype=np.int32)), t(np.array(first, dtype=np.int32))
    d_ls, d_nr = t(np.array(b_ls, dtype=np.int32)), t(np.array(b_nr, dtype=np.int32))

    # sizing passes, then the arenas
    p_off, p_sz, p_st, chosen = i64(nblk + 1), i32(nblk), i32(nblk), i32(n)
    dc.tok3_pack(d_first, d_in, d_coff, d_csz, d_cid, d_ls, d_nr, None, p_off, p_sz, p_st, NINE, max_col, chosen=chosen, total_col_size=total)
    torch.cuda.synchronize()
    packed = torch.empty(int(p_off[-1]) + 64, dtype=torch.uint8, device=dev)
    s_off, s_sz, s_st = i64(n + 1), i32(n), i32(n)
    # (every column's winner, the duplicates' too: more than the containers hold; the bound of pack's own arena)
    streams = torch.empty(int(1.05 * total) + 900 * n + 64, dtype=torch.uint8, device=dev)
    cols = torch.empty(2 * total + 64, dtype=torch.uint8, device=dev)                # (type columns come on top)
    u_off, u_sz, u_st, u_nc, u_ls, u_nr = i64(nblk + 1), i32(nblk), i32(nblk), i32(nblk), i32(nblk), i32(nblk)
    u_id, u_coff, u_csz = i32(nblk * maxc), i64(nblk * maxc), i32(nblk * maxc)
    back = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    b_off, b_sz, b_st = i64(n + 1), i32(n), i32(n)
    max_cont = 1 << 20

    calls = {
        "tok3_pack": lambda: dc.tok3_pack(d_first, d_in, d_coff, d_csz, d_cid, d_ls, d_nr, packed, p_off, p_sz, p_st, NINE, max_col,
                                          chosen=chosen, total_col_size=total),
        "best_packed": lambda: dc.compress_best_packed(d_in, d_coff, d_csz, streams, s_off, s_sz, s_st, NINE, max_col, chosen=chosen,
                                                       total_in_size=total),
        "tok3_unpack": lambda: dc.tok3_unpack(packed, p_off, p_sz, cols, u_off, u_sz, u_st, u_nc, u_ls, u_nr, u_id, u_coff, u_csz,
                                              maxc, max_cont, max_col),
        "uncompress_packed": lambda: dc.uncompress_packed(streams, s_off, s_sz, back, b_off, b_sz, b_st, max_cont, max_col),
    }
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
    assert (p_st == 0).all(), 'pack'
    assert (s_st == 0).all(), 'best_packed'
    assert (b_st == 0).all(), 'uncompress_packed'
    refused = int((u_st != 0).sum())                 # containers whose last column is a duplicate: the reference refuses them too
    res = {"blocks": nblk, "columns": n, "column_bytes": total, "container_bytes": int(p_off[-1]), "stream_bytes": int(s_off[-1]),
           "unpack_refused": refused, "max_columns": maxc, "passes": args.passes,
           "workspace_bytes": dc.workspace_bytes(), "workspace_bytes_per_column": dc.workspace_bytes() / n}
    for k, v in ms.items():
        res[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
