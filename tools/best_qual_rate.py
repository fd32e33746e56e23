#!/usr/bin/env python3
"""Rate of best-of across rANS 4x16, arith_dynamic and fqzcomp_qual for quality blocks (include/rans4x16_hip.h part 2n),
beside tools/best_any_rate.py and tools/fqz_best_rate.py and with the latter's batches: the slice of one reference-made
fixture (q40+dir: 100,000 qualities in 1,000 records), repeated, the blocks independent, the model slots sized for the
fixture's max_sym.  The list is a writer's: {rANS 1, arith 1, FQZ|0, FQZ|1, FQZ|2, FQZ|3}.  One JSON line per batch size.

Two ways to the same dense arena, alternating pass by pass after a warm-up pass of each, the median and every pass reported:
  one_call   rans4x16_hip_compress_best_qual_packed_dev: one enqueue, nothing read back
  baseline   what the parent commit offers for the same job: rans4x16_hip_compress_best_any_packed_dev under {rANS 1,
             arith 1} into one arena and rans4x16_hip_fqz_compress_best_packed_dev under [0, 1, 2, 3] into another, both
             size arrays (with their offsets and methods) read back, the comparison on the host (smaller size, on a tie the
             method that stands earlier in the list), one gather of the winners into one arena on the device
Both are timed by a host clock around work that ends in a device synchronise (the baseline has a read-back in its middle);
the one call also by HIP events.  Every pass's arena, offsets and methods are compared on the device, one way against the
other; the warm-up pass of the one call is also decoded again by rans4x16_hip_uncompress_qual_packed_dev and compared with
the input and the record lengths.

--only one_call | baseline runs that way alone, for a kernel trace in a run of its own (rocprofv3 --kernel-trace --stats):
the new kernels' share of the call is the time of k_bq_pick and k_bq_gather over the time of all kernels."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ARITH, FQZ, MASK = 1 << 24, 3 << 24, 0x0F000000
STRATS = [0, 1, 2, 3]
PAIR = [1, ARITH | 1]
METHODS = PAIR + [FQZ | s for s in STRATS]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default="q40+dir")
    ap.add_argument("--blocks", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--only", choices=("one_call", "baseline"), default=None)
    a = ap.parse_args()
    import torch
    import fqz_enc_model as E
    import htscodecs_amd as H
    assert torch.cuda.is_available(), "best_qual_rate.py measures on a GPU"
    dc = H.DeviceCodec(0)
    dev = dc.dev
    slices = {f[0]: f for f in E.fixture_slices()}
    fn, _, stream0, raw, lens, flags = slices["%s.0" % a.fixture]
    dc.set_fqz_limits(max_sym=H.fqz_scan(stream0)[1]["max_sym"])
    pos = {m: j for j, m in enumerate(METHODS)}
    cap = H.fqz_compress_cap(len(raw), len(lens), H.fqz_pick_cap())
    up = lambda arr: torch.from_numpy(np.asarray(arr, dtype=np.int64).astype(np.uint32).view(np.int32).copy()).to(dev)
    u8 = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(dev)
    size, nrec = len(raw), len(lens)
    for n in a.blocks:
        stride_in = (size + 255) // 256 * 256
        d_in = torch.zeros(n * stride_in + 64, dtype=torch.uint8, device=dev)
        d_in[:n * stride_in].view(n, stride_in)[:, :size] = u8(raw)
        d_len, d_fl = up(lens * n), up(flags * n)
        in_off = torch.arange(n, dtype=torch.int64, device=dev) * stride_in
        rec_off = torch.arange(n, dtype=torch.int64, device=dev) * nrec
        in_size, nrecs = torch.full((n,), size, dtype=torch.int32, device=dev), torch.full((n,), nrec, dtype=torch.int32, device=dev)
        room = n * ((cap + 255) // 256 * 256)
        i32 = lambda: torch.full((n,), -1, dtype=torch.int32, device=dev)
        off64 = lambda: torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
        d_out, off, osz, st, ch = torch.zeros(room, dtype=torch.uint8, device=dev), off64(), i32(), i32(), i32()
        d_lo = torch.full_like(d_len, -1)
        # the baseline's: one allocation for both calls' arenas (the gather then indexes one tensor) and the dense result
        two = torch.zeros(2 * room, dtype=torch.uint8, device=dev) if a.only != "one_call" else None
        off2, osz2, st2, ch2 = (off64(), off64()), (i32(), i32()), (i32(), i32()), (i32(), i32())
        d_lo2 = torch.full_like(d_len, -1)
        dense = torch.zeros(room, dtype=torch.uint8, device=dev) if a.only != "one_call" else None

        def one_call():
            dc.compress_best_qual_packed(d_in, in_off, in_size, d_len, d_fl, rec_off, nrecs, d_out, off, osz, st, METHODS, size, nrec,
                                         chosen=ch, d_len_out=d_lo, total_in_size=n * size)
            return d_out, off, ch

        def baseline():
            dc.compress_best_any_packed(d_in, in_off, in_size, two[:room], off2[0], osz2[0], st2[0], PAIR, size, chosen=ch2[0],
                                        total_in_size=n * size)
            dc.fqz_compress_best_packed(d_in, in_off, in_size, d_len, d_fl, rec_off, nrecs, two[room:], off2[1], osz2[1], st2[1], STRATS,
                                        size, nrec, chosen=ch2[1], d_len_out=d_lo2)
            # the read-back: sizes, offsets and methods of both
            sz = [osz2[c].cpu().numpy().astype(np.int64) for c in (0, 1)]
            of = [off2[c].cpu().numpy() for c in (0, 1)]
            won = [ch2[c].cpu().numpy() for c in (0, 1)]
            assert (st2[0].cpu().numpy() == 0).all() and (st2[1].cpu().numpy() == 0).all()
            # the comparison on the host
            p_ra = np.array([pos[int(m)] for m in won[0]])
            p_f = np.array([pos[FQZ | STRATS[int(j)]] for j in won[1]])
            fqz = (sz[1] < sz[0]) | ((sz[1] == sz[0]) & (p_f < p_ra))
            sizes = np.where(fqz, sz[1], sz[0])
            src = np.where(fqz, of[1][:-1] + room, of[0][:-1])
            dst = np.concatenate(([0], np.cumsum(sizes)))
            # the second gather, on the device: every result byte's source index
            d_sizes = torch.from_numpy(sizes).to(dev)
            shift = torch.repeat_interleave(torch.from_numpy(src - dst[:-1]).to(dev), d_sizes)
            total = int(dst[-1])
            idx = torch.arange(total, dtype=torch.int64, device=dev) + shift
            torch.index_select(two, 0, idx, out=dense[:total])
            chosen = np.where(fqz, np.array([FQZ | STRATS[int(j)] for j in won[1]]), won[0]).astype(np.int32)
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
                tags = ch.bitwise_and(MASK)
                wins = {"rans": int(tags.eq(0).sum().item()), "arith": int(tags.eq(ARITH).sum().item()), "fqz": int(tags.eq(FQZ).sum().item())}
                back, boff, bsz, bst, bnrec = torch.zeros(n * size, dtype=torch.uint8, device=dev), off64(), i32(), i32(), i32()
                blen = torch.full_like(d_len, -1)
                dc.uncompress_qual_packed(d_out, off, osz, ch, back, boff, bsz, bst, int(osz.max().item()), size, d_len=blen, len_off=rec_off,
                                          len_cap=nrecs, nrec=bnrec)
                torch.cuda.synchronize()
                assert bst.eq(0).all().item() and torch.equal(back.view(n, size), d_in[:n * stride_in].view(n, stride_in)[:, :size]), \
                    "the round trip differs from the input"
                by_fqz = tags.eq(FQZ)
                assert torch.equal(bnrec, torch.where(by_fqz, nrecs, torch.zeros_like(nrecs))), "the record counts differ"
                assert torch.equal(blen.view(n, nrec)[by_fqz], d_len.view(n, nrec)[by_fqz]), "the record lengths differ"
        out = {"fixture": a.fixture, "blocks": n, "block_bytes": size, "methods": METHODS, "wins": wins,
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
    dc.set_fqz_limits(0, 0)


if __name__ == "__main__":
    main()
