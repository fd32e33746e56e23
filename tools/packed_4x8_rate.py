#!/usr/bin/env python3
"""rANS 4x8: rans4x8_hip_compress_packed_dev against rans4x8_hip_compress_dev, and rans4x8_hip_compress_best_packed_dev
against what a caller does without it (two slot-call encodes, then its own pick and gather - emulated by one device copy
of as many bytes as the winners have), on the same blocks: all forms in one process, alternating, timed with device
events; and what each makes the caller hold.

    python tools/packed_4x8_rate.py [--blocks 7680] [--size 1048576] [--order 1] [--passes 5] [--warmup 2] [--no-best] [--out FILE]
    rocprofv3 --kernel-trace --stats ... -- python tools/packed_4x8_rate.py --only slot_call | packed_call ...

--only FORM runs that form alone, for a kernel trace in which every launch belongs to it: the packed call then sizes
its arena with its own sizing pass (no arena, capacity 0) and no slot is allocated.

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7680)
    ap.add_argument("--size", type=int, default=1 << 20)
    ap.add_argument("--order", type=int, default=1)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-best", action="store_true")
    ap.add_argument("--only", choices=("slot_call", "packed_call"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import datagen
    import htscodecs_amd as H
    if not torch.cuda.is_available():
        sys.exit("packed_4x8_rate: no GPU (there is no CPU path to time)")
    n, size, order = args.blocks, args.size, args.order
    dc = H.DeviceCodec(0)
    dev = dc.dev
    t = lambda a: torch.from_numpy(a).to(dev)
    text = datagen.tile("q40+dir", 64 << 20, 1)
    reps = -(-n * size // len(text))
    d_in = t(text).repeat(reps)[:n * size].contiguous()
    cap = dc.L.rans4x8_hip_compress_bound(size)
    slot = (cap + 255) // 256 * 256
    in_off, in_size = t(np.arange(n, dtype=np.int64) * size), t(np.full(n, size, dtype=np.int32))
    out_off, caps = t(np.arange(n, dtype=np.int64) * slot), t(np.full(n, cap, dtype=np.int32))
    new_i32 = lambda: torch.zeros(n, dtype=torch.int32, device=dev)
    s_osz, s_st, p_osz, p_st, b_osz, b_st, chosen = (new_i32() for _ in range(7))
    total = n * size
    p_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    slots = need = best_need = None

    def slot_call(o=order):
        dc.compress_4x8(d_in, in_off, in_size, slots, out_off, caps, s_osz, s_st, o, size)

    def packed_call():
        dc.compress_packed_4x8(d_in, in_off, in_size, dense, p_off, p_osz, p_st, order, size)

    if args.only != "packed_call":
        slots = torch.empty(n * slot, dtype=torch.uint8, device=dev)
        slot_call()
        torch.cuda.synchronize()
        assert (s_st == 0).all()
        need = int(s_osz.to(torch.int64).sum())
    else:
        rc = dc.L.rans4x8_hip_compress_packed_dev(dc.ctx.h, n, d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(), None, 0,
                                                  p_off.data_ptr(), p_osz.data_ptr(), p_st.data_ptr(), order, None, size,
                                                  dc._stream())
        assert rc == 0, dc.ctx.error()
        torch.cuda.synchronize()
        need = int(p_off[-1])
    forms = {}
    if args.only != "packed_call":
        forms["slot_call"] = slot_call
    if args.only != "slot_call":
        dense = torch.empty(need + 64, dtype=torch.uint8, device=dev)
        packed_call()
        torch.cuda.synchronize()
        assert (p_st == 0).all() and int(p_off[-1]) == need
        if slots is not None:
            assert torch.equal(p_osz, s_osz)
            offs = p_off.cpu().numpy()
            for i in range(0, n, max(1, n // 64)):
                o, sz = int(offs[i]), int(offs[i + 1] - offs[i])
                assert torch.equal(dense[o:o + sz], slots[i * slot:i * slot + sz]), i
        forms["packed_call"] = packed_call
    if not args.no_best and not args.only:
        def best_packed():
            dc.compress_best_4x8(d_in, in_off, in_size, dense, p_off, b_osz, b_st, [0, 1], size, chosen=chosen, packed=True)

        best_packed()
        torch.cuda.synchronize()
        assert (b_st == 0).all()
        best_need = int(p_off[-1])
        assert best_need <= need + 64
        gathered = torch.empty(best_need, dtype=torch.uint8, device=dev)

        def two_slot_calls_pick_gather():
            slot_call(0)
            slot_call(1)
            gathered.copy_(slots[:best_need])            # the caller's gather of the winners: as many bytes, one device copy

        forms["best_packed_call"] = best_packed
        forms["two_slot_calls_pick_gather"] = two_slot_calls_pick_gather

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(args.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(args.passes):
        for name, fn in forms.items():
            ms[name].append(timed(fn))
    res = {"codec": "rans4x8", "blocks": n, "block_bytes": size, "order": order, "passes": args.passes,
           "caller_output_bytes": {"slots": n * slot, "dense": need, "dense_best": best_need},
           "context_bytes": {"workspace": dc.workspace_bytes()}}
    for name, v in ms.items():
        v = np.array(v)
        res[name] = {"median_ms": round(float(np.median(v)), 3), "best_ms": round(float(v.min()), 3),
                     "worst_ms": round(float(v.max()), 3), "input_mb_per_s_median": round(total / 1e3 / float(np.median(v)), 1)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
