#!/usr/bin/env python3
"""rans4x16_hip_compress_packed_dev against rans4x16_hip_compress_dev_sized on the same blocks: both calls in one
process, alternating, timed with device events; and what each makes the caller and the context hold.

    python tools/packed_dev_rate.py [--blocks 23040] [--size 1048576] [--order 1] [--passes 5] [--warmup 2] [--out FILE]

Prints one JSON line.  A third form is timed when tools/probe/libpack_gather.so exists (tools/pack_gather.hip: the
host-batch pipeline's gather kernel, k_pack_results, behind one C entry point): the slot call followed by that gather of
its results into the dense arena, the descriptors built on the device from the sizes the slot call wrote."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=23040)
    ap.add_argument("--size", type=int, default=1 << 20)
    ap.add_argument("--order", type=int, default=1)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import datagen
    import htscodecs_amd as H
    if not torch.cuda.is_available():
        sys.exit("packed_dev_rate: no GPU (there is no CPU path to time)")
    n, size, order = args.blocks, args.size, args.order
    dc = H.DeviceCodec(0)
    dev = dc.dev
    t = lambda a: torch.from_numpy(a).to(dev)
    text = datagen.tile("q40+dir", 64 << 20, 1)
    reps = -(-n * size // len(text))
    d_in = t(text).repeat(reps)[:n * size].contiguous()
    cap = H.rans_compress_bound_4x16(size, order)
    slot = (cap + 255) // 256 * 256
    in_off, in_size = t(np.arange(n, dtype=np.int64) * size), t(np.full(n, size, dtype=np.int32))
    out_off, caps = t(np.arange(n, dtype=np.int64) * slot), t(np.full(n, cap, dtype=np.int32))
    new_i32 = lambda: torch.zeros(n, dtype=torch.int32, device=dev)
    s_osz, s_st, p_osz, p_st = new_i32(), new_i32(), new_i32(), new_i32()
    slots = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    total = n * size

    def slot_call():
        dc.compress(d_in, in_off, in_size, slots, out_off, caps, s_osz, s_st, order, size, total_in_size=total)

    slot_call()
    torch.cuda.synchronize()
    assert (s_st == 0).all()
    need = int(s_osz.to(torch.int64).sum())
    dense = torch.empty(need, dtype=torch.uint8, device=dev)
    p_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)

    def packed_call():
        dc.compress_packed(d_in, in_off, in_size, dense, p_off, p_osz, p_st, order, size, total_in_size=total)

    free0 = torch.cuda.mem_get_info(dev)[0]
    packed_call()
    torch.cuda.synchronize()
    arena = free0 - torch.cuda.mem_get_info(dev)[0]                  # the packed arena (the workspace is in place already)
    assert (p_st == 0).all() and torch.equal(p_osz, s_osz) and int(p_off[-1]) == need
    offs = p_off.cpu().numpy()
    for i in range(0, n, max(1, n // 64)):
        o, sz = int(offs[i]), int(offs[i + 1] - offs[i])
        assert torch.equal(dense[o:o + sz], slots[i * slot:i * slot + sz]), i

    probe = os.path.join(ROOT, "tools", "probe", "libpack_gather.so")
    gather = C.CDLL(probe).pack_gather if os.path.exists(probe) else None
    dense2 = torch.empty(need, dtype=torch.uint8, device=dev) if gather else None

    def slot_then_gather():
        slot_call()
        sz = s_osz.to(torch.int64)
        desc = torch.stack((out_off, torch.cumsum(sz, 0) - sz, sz), dim=1).contiguous()     # {src, dst, len | pad << 32}
        rc = gather(C.c_void_p(slots.data_ptr()), C.c_void_p(dense2.data_ptr()), C.c_void_p(desc.data_ptr()), n,
                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == 0

    if gather:
        slot_then_gather()
        torch.cuda.synchronize()
        assert torch.equal(dense2, dense), "slot call + gather and the packed call differ"

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    forms = {"slot_call": slot_call, "packed_call": packed_call}
    if gather:
        forms["slot_call_then_gather"] = slot_then_gather
    for _ in range(args.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(args.passes):
        for name, fn in forms.items():
            ms[name].append(timed(fn))
    res = {"blocks": n, "block_bytes": size, "order": order, "passes": args.passes,
           "caller_output_bytes": {"slots": n * slot, "dense": need},
           "context_bytes": {"workspace": dc.workspace_bytes(), "packed_arena_as_allocated": int(arena)}}
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
