#!/usr/bin/env python3
"""Rate of best-of across codecs, rANS 4x16 against arith_dynamic (include/rans4x16_hip.h part 2m), beside
tools/fqz_best_rate.py.  Two batches, one JSON line each:
  64k   1,024 blocks of 64 KiB cycling the q4 / q8 / q40+dir texts under {rANS 0, 1, 65, 193; arith 0, 1, 65, 193}
  4k    4,096 blocks of 4 KiB of the same texts under {rANS 0, 1; arith 0, 1}

Two ways to the same dense arena, alternating pass by pass after a warm-up pass of each, the median and every pass reported:
  one_call   rans4x16_hip_compress_best_any_packed_dev: one enqueue, nothing read back
  baseline   what a caller of the single-codec interface has to do: rans4x16_hip_compress_best_packed_dev and
             rans4x16_hip_arith_compress_best_packed_dev into two arenas, both size and method arrays read back, the pick on
             the host (smaller size, on a tie the method that stands earlier in the list), one gather of the winners into one
             arena on the device
Both are timed by a host clock around work that ends in a device synchronise (the baseline has a read-back in its middle);
the one call also by HIP events.  Every pass's arena, offsets and methods are compared on the device, one way against the
other; the warm-up pass of the one call is also decoded again by rans4x16_hip_uncompress_any_packed_dev and compared with the
input.

--only one_call | baseline runs that way alone, for a kernel trace in a run of its own (rocprofv3 --kernel-trace --stats):
the share of the call that picks across codecs is the time of k_bq_pick and k_bq_gather - the kernels parts 2m and 2n
share - over the time of all kernels."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ARITH = 1 << 24
BATCHES = {"64k": (1024, 65536, (0, 1, 65, 193)), "4k": (4096, 4096, (0, 1))}
TEXTS = ("q4", "q8", "q40+dir")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", default=["64k", "4k"], choices=sorted(BATCHES))
    ap.add_argument("--blocks", type=int, default=None, help="blocks per batch instead of the batch's own number")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--only", choices=("one_call", "baseline"), default=None)
    a = ap.parse_args()
    import torch
    import datagen
    import htscodecs_amd as H
    assert torch.cuda.is_available(), "best_any_rate.py measures on a GPU"
    dc = H.DeviceCodec(0)
    dev = dc.dev
    for name in a.batches:
        n, size, orders = BATCHES[name]
        n = a.blocks or n
        methods = list(orders) + [ARITH | o for o in orders]
        pos = {m: j for j, m in enumerate(methods)}
        texts = [torch.from_numpy(datagen.tile(t, size, 1).copy()).to(dev) for t in TEXTS]
        d_in = torch.zeros(n * size + 64, dtype=torch.uint8, device=dev)
        for i, t in enumerate(texts):
            d_in[:n * size].view(n, size)[i::len(texts)] = t
        in_off = torch.arange(n, dtype=torch.int64, device=dev) * size
        in_size = torch.full((n,), size, dtype=torch.int32, device=dev)
        room = n * (size + size // 16 + 1024)
        i32 = lambda: torch.full((n,), -1, dtype=torch.int32, device=dev)
        off64 = lambda: torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
        d_out, off, osz, st, ch = torch.zeros(room, dtype=torch.uint8, device=dev), off64(), i32(), i32(), i32()
        # the baseline's: one allocation for both codecs' arenas (the gather then indexes one tensor) and the dense result
        two = torch.zeros(2 * room, dtype=torch.uint8, device=dev) if a.only != "one_call" else None
        off2, osz2, st2, ch2 = (off64(), off64()), (i32(), i32()), (i32(), i32()), (i32(), i32())
        dense = torch.zeros(room, dtype=torch.uint8, device=dev) if a.only != "one_call" else None

        def one_call():
            dc.compress_best_any_packed(d_in, in_off, in_size, d_out, off, osz, st, methods, size, chosen=ch, total_in_size=n * size)
            return d_out, off, ch

        def baseline():
            dc.compress_best_packed(d_in, in_off, in_size, two[:room], off2[0], osz2[0], st2[0], list(orders), size, chosen=ch2[0],
                                    total_in_size=n * size)
            dc.arith_compress_best_packed(d_in, in_off, in_size, two[room:], off2[1], osz2[1], st2[1], list(orders), size, chosen=ch2[1],
                                          total_in_size=n * size)
            # the read-back: sizes, offsets and methods of both
            sz = [osz2[c].cpu().numpy().astype(np.int64) for c in (0, 1)]
            of = [off2[c].cpu().numpy() for c in (0, 1)]
            won = [ch2[c].cpu().numpy() for c in (0, 1)]
            assert (st2[0].cpu().numpy() == 0).all() and (st2[1].cpu().numpy() == 0).all()
            # the pick on the host
            p_r = np.array([pos[int(m)] for m in won[0]])
            p_a = np.array([pos[ARITH | int(m)] for m in won[1]])
            arith = (sz[1] < sz[0]) | ((sz[1] == sz[0]) & (p_a < p_r))
            sizes = np.where(arith, sz[1], sz[0])
            src = np.where(arith, of[1][:-1] + room, of[0][:-1])
            dst = np.concatenate(([0], np.cumsum(sizes)))
            # the gather on the device: every result byte's source index
            d_sizes = torch.from_numpy(sizes).to(dev)
            shift = torch.repeat_interleave(torch.from_numpy(src - dst[:-1]).to(dev), d_sizes)
            total = int(dst[-1])
            idx = torch.arange(total, dtype=torch.int64, device=dev) + shift
            torch.index_select(two, 0, idx, out=dense[:total])
            chosen = np.where(arith, won[1] | ARITH, won[0]).astype(np.int32)
            return dense, torch.from_numpy(dst).to(dev), torch.from_numpy(chosen).to(dev)

        ways = [w for w in (("one_call", one_call), ("baseline", baseline)) if a.only in (None, w[0])]
        wall = {w: [] for w, _ in ways}
        events = []
        wins = None
        for p in range(a.passes + 1):                                # pass 0 warms up (and grows the arenas)
            got = {}
            for w, call in ways:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                res = call()
                e1.record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                total = int(res[1][-1].item())
                got[w] = (res[0][:total].clone(), res[1].clone(), res[2].clone())
                if p:
                    wall[w].append((t1 - t0) * 1e3)
                    if w == "one_call":
                        events.append(e0.elapsed_time(e1))
            if len(got) == 2:
                for x, y, what in zip(got["one_call"], got["baseline"], ("bytes", "offsets", "methods")):
                    assert torch.equal(x, y), "pass %d: the two ways differ in their %s" % (p, what)
            if p == 0 and "one_call" in got:
                assert st.eq(0).all().item(), "a block failed"
                wins = int(ch.ge(ARITH).sum().item())
                back, boff, bsz, bst = torch.zeros(n * size, dtype=torch.uint8, device=dev), off64(), i32(), i32()
                dc.uncompress_any_packed(d_out, off, osz, ch, back, boff, bsz, bst, int(osz.max().item()), size)
                torch.cuda.synchronize()
                assert bst.eq(0).all().item() and torch.equal(back, d_in[:n * size]), "the round trip differs from the input"
        out = {"batch": name, "blocks": n, "block_bytes": size, "methods": methods, "arith_wins": wins,
               "out_bytes": int(off[-1].item()) if "one_call" in wall else None}
        for w, _ in ways:
            out["ms_" + w] = round(float(np.median(wall[w])), 3)
            out["ms_all_" + w] = [round(x, 3) for x in wall[w]]
        if events:
            out["ms_one_call_events"] = round(float(np.median(events)), 3)
            out["one_call_GBps"] = round(n * size / out["ms_one_call"] / 1e6, 3)
        if len(ways) == 2:
            out["one_call_over_baseline"] = round(out["ms_one_call"] / out["ms_baseline"], 4)
        print(json.dumps(out), flush=True)
        del d_in, d_out, two, dense


if __name__ == "__main__":
    main()
