#!/usr/bin/env python3
"""Rate of the device-resident best-of-nine call (rans4x16_hip_compress_best_dev) against what a device-resident caller
has to do without it: one rans4x16_hip_compress_dev call per method into nine arenas, the sizes read back, the winners
copied device to device.  Both forms in one process on the same seeded inputs, alternating, timed with device events
around everything a pass does (the baseline's read-back and copies included).

    python tools/best_dev_rate.py [--blocks 4096] [--size 65536] [--passes 10] [--warmup 2] [--out FILE]

Prints one JSON line per input kind (q8 tiles; little-endian uint32 columns, where the stripe method wins)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NINE = [0, 1, 128, 129, 64, 65, 192, 193, 201]           # tokenise_name3.c:1259


def make_inputs(kind, n, size):
    import datagen
    if kind == "q8":
        return np.concatenate([datagen.tile("q8", size, k) for k in range(n)])
    rs = np.random.RandomState(11)
    return rs.randint(0, 300, n * size // 4).astype("<u4").view(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--size", type=int, default=65536)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import htscodecs_amd as H
    if not torch.cuda.is_available():
        sys.exit("best_dev_rate: no GPU (there is no CPU path to time)")
    n, size, k = args.blocks, args.size, len(NINE)
    dc = H.DeviceCodec(0)
    dev = dc.dev
    cap = max(H.rans_compress_bound_4x16(size, m) for m in NINE)
    slot = (cap + 255) // 256 * 256
    t = lambda a: torch.from_numpy(a).to(dev)
    in_off = t(np.arange(n, dtype=np.int64) * size)
    in_size = t(np.full(n, size, dtype=np.int32))
    out_off_np = np.arange(n, dtype=np.int64) * slot
    out_off, caps = t(out_off_np), t(np.full(n, cap, dtype=np.int32))
    new_i32 = lambda: torch.zeros(n, dtype=torch.int32, device=dev)
    out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    osz, st, chosen = new_i32(), new_i32(), new_i32()
    arenas = [torch.empty(n * slot, dtype=torch.uint8, device=dev) for _ in NINE]
    b_out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    b_osz, b_st = [new_i32() for _ in NINE], [new_i32() for _ in NINE]
    lines, held, ws = [], 0, 0
    for kind in ("q8", "uint32"):
        d_in = t(make_inputs(kind, n, size))
        total = n * size

        def one_call():
            dc.compress_best(d_in, in_off, in_size, out, out_off, caps, osz, st, NINE, size, chosen=chosen, total_in_size=total)

        def baseline(copies=True):
            for j, m in enumerate(NINE):
                dc.compress(d_in, in_off, in_size, arenas[j], out_off, caps, b_osz[j], b_st[j], m, size, total_in_size=total)
            sizes = torch.stack(b_osz).cpu().numpy().astype(np.int64)          # the read-back (waits for the nine calls)
            ok = torch.stack(b_st).cpu().numpy() == 0
            sizes[~ok] = 1 << 40
            win = sizes.argmin(axis=0)                                          # the first of equals, as the loop keeps it
            if copies:
                for i in range(n):
                    o, sz = int(out_off_np[i]), int(sizes[win[i], i])
                    b_out[o:o + sz].copy_(arenas[win[i]][o:o + sz], non_blocking=True)
            return win, sizes

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        free0 = torch.cuda.mem_get_info(dev)[0]
        one_call()
        torch.cuda.synchronize()
        if kind == "q8":                                                        # (the second kind finds both arenas in place)
            held = free0 - torch.cuda.mem_get_info(dev)[0]                      # workspace + candidate arena, as the driver sees it
            ws = dc.workspace_bytes()
        dc.set_option("route_count", 1)
        dc.route_read("launch")
        one_call()
        chunks = sum(dc.route_read("launch").values())                          # chain launches of the inner calls
        dc.set_option("route_count", 0)
        # same results first (same inputs, same methods): sizes, winners, bytes of a sample
        win, sizes = baseline()
        torch.cuda.synchronize()
        want_sz = sizes[win, np.arange(n)]
        assert (st.cpu().numpy() == 0).all()
        assert (osz.cpu().numpy() == want_sz).all(), "sizes differ between the one-call form and the baseline"
        assert (chosen.cpu().numpy() == np.array(NINE)[win]).all(), "winners differ"
        for i in range(0, n, max(1, n // 64)):
            o = int(out_off_np[i])
            assert torch.equal(out[o:o + int(want_sz[i])], b_out[o:o + int(want_sz[i])]), i
        for _ in range(args.warmup):
            one_call(); baseline(); baseline(False)
        torch.cuda.synchronize()
        ms = {"one_call": [], "baseline": [], "baseline_without_copies": []}
        for _ in range(args.passes):                                            # alternating: the host is shared
            ms["one_call"].append(timed(one_call))
            ms["baseline"].append(timed(baseline))
            ms["baseline_without_copies"].append(timed(lambda: baseline(False)))
        res = {"input": kind, "blocks": n, "block_bytes": size, "methods": NINE, "passes": args.passes,
               "winners": {str(NINE[j]): int((win == j).sum()) for j in range(k) if (win == j).any()},
               "workspace_mb": ws >> 20, "arena_mb": max(held - ws, 0) >> 20, "inner_chain_launches": chunks}
        for name, v in ms.items():
            v = np.array(v)
            res[name] = {"median_ms": round(float(np.median(v)), 3), "best_ms": round(float(v.min()), 3),
                         "worst_ms": round(float(v.max()), 3), "input_mb_per_s_median": round(total / 1e3 / float(np.median(v)), 1)}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
