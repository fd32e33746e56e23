#!/usr/bin/env python3
"""Rate of best-of-four strategies for fqzcomp_qual encoding (include/rans4x16_hip.h part 2l), beside
tools/fqz_pick_rate.py and tools/fqz_enc_rate.py and with their batches: the text of one reference-made fixture, repeated,
the blocks independent, the model slots sized for the fixture's max_sym.  One JSON line per batch size.

Two ways to the same bytes, alternating pass by pass after a warm-up pass of each, the median and every pass reported:
  one_call   rans4x16_hip_fqz_compress_best_dev with the list [0, 1, 2, 3]: one enqueue, nothing read back
  baseline   what a caller could do before: four rans4x16_hip_fqz_compress_pick_dev calls into four bound-sized slots a
             block, the four size arrays read back, the winners picked on the host, one gather of the winners' slots on
             the device.  --baseline-lib PATH runs these calls on another build of the library (the parent commit's);
             the default is this build's.
Both are timed by a host clock around work that ends in a device synchronise (the baseline has a read-back in its middle);
the one call also by HIP events.  Every pass's winners are compared with the reference's smallest stream on the device.

--only one_call | baseline runs that way alone, for a kernel trace in a run of its own (rocprofv3 --kernel-trace --stats):
the pick's share of either is the time of the k_fqp_* and k_fqb_store kernels over the time of all kernels."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
STRATS = [0, 1, 2, 3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default="q40+dir")
    ap.add_argument("--blocks", type=int, nargs="+", default=[1, 256, 1024])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--only", choices=("one_call", "baseline"), default=None)
    a = ap.parse_args()
    import torch
    import fqz_enc_model as E
    import htscodecs_amd as H
    from htscodecs_amd import lib as hlib
    assert torch.cuda.is_available(), "fqz_best_rate.py measures on a GPU"
    dc = H.DeviceCodec(0)
    dev = dc.dev
    slices = {f[0]: f for f in E.fixture_slices()}
    streams = [slices["%s.%d" % (a.fixture, s)][2] for s in STRATS]
    fn, _, _, raw, lens, flags = slices["%s.0" % a.fixture]
    win = min(range(4), key=lambda s: len(streams[s]))              # (min keeps the first of equals, as the call does)
    max_sym = H.fqz_scan(streams[0])[1]["max_sym"]
    dc.set_fqz_limits(max_sym=max_sym)
    # the baseline's library and context: this build's, or the one given
    base = hlib.load()
    if a.baseline_lib:
        base = C.CDLL(os.path.abspath(a.baseline_lib))
        for name in ("rans4x16_hip_create", "rans4x16_hip_set_fqz_limits", "rans4x16_hip_fqz_compress_pick_dev", "rans4x16_hip_last_error"):
            getattr(base, name).restype, getattr(base, name).argtypes = hlib.SIGNATURES[name]
    bctx = base.rans4x16_hip_create(0)
    assert bctx and base.rans4x16_hip_set_fqz_limits(bctx, 0, max_sym) == 0
    cap = H.fqz_compress_cap(len(raw), len(lens), H.fqz_pick_cap())
    up = lambda arr: torch.from_numpy(np.asarray(arr, dtype=np.int64).astype(np.uint32).view(np.int32).copy()).to(dev)
    u8 = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(dev)
    want = u8(streams[win])
    for n in a.blocks:
        stride_in, stride_out, nrec = (len(raw) + 255) // 256 * 256, (cap + 255) // 256 * 256, len(lens)
        d_in = torch.zeros(n * stride_in + 64, dtype=torch.uint8, device=dev)
        d_in[:n * stride_in].view(n, stride_in)[:, :len(raw)] = u8(raw)
        d_len, d_fl = up(lens * n), up(flags * n)
        i64 = lambda v: torch.arange(n, dtype=torch.int64, device=dev) * v
        i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)
        in_off, in_size, rec_off, nrecs, out_off, out_cap = i64(stride_in), i32(len(raw)), i64(nrec), i32(nrec), i64(stride_out), i32(cap)
        d_out = torch.zeros(n * stride_out, dtype=torch.uint8, device=dev)
        d_osz, d_st, d_ch = i32(-1), i32(-1), i32(-1)
        # the baseline's: four slots a block, four size and status arrays
        d_out4 = torch.zeros(4 * n * stride_out, dtype=torch.uint8, device=dev) if a.only != "one_call" else None
        d_osz4, d_st4 = torch.full((4, n), -1, dtype=torch.int32, device=dev), torch.full((4, n), -1, dtype=torch.int32, device=dev)
        rows = torch.arange(n, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def one_call():
            dc.fqz_compress_best(d_in, in_off, in_size, d_len, d_fl, rec_off, nrecs, d_out, out_off, out_cap, d_osz, d_st, STRATS,
                                 len(raw), nrec, vers=4, chosen=d_ch)
            return d_out.view(n, stride_out), d_osz, d_ch

        def baseline():
            for s in STRATS:
                rc = base.rans4x16_hip_fqz_compress_pick_dev(
                    bctx, n, d_in.data_ptr(), in_off.data_ptr(), in_size.data_ptr(), d_len.data_ptr(), d_fl.data_ptr(), rec_off.data_ptr(),
                    nrecs.data_ptr(), 4, s, None, d_out4[s * n * stride_out:].data_ptr(), out_off.data_ptr(), out_cap.data_ptr(),
                    d_osz4[s].data_ptr(), d_st4[s].data_ptr(), len(raw), nrec, stream)
                assert rc == 0, base.rans4x16_hip_last_error(bctx)
            sizes, sts = d_osz4.cpu().numpy(), d_st4.cpu().numpy()      # the read-back
            assert (sts == 0).all()
            best = torch.from_numpy(sizes.argmin(axis=0)).to(dev)       # (argmin keeps the first of equals)
            dense = d_out4.view(4, n, stride_out)[best, rows]           # the winners' slots, gathered on the device
            return dense, torch.from_numpy(sizes.min(axis=0)).to(dev), best.to(torch.int32)

        def check(res):
            out, osz, ch = res
            assert osz.eq(len(streams[win])).all().item() and ch.eq(win).all().item(), "another winner than the reference's"
            assert out[:, :len(streams[win])].eq(want).all().item(), "bytes differ"

        ways = [w for w in (("one_call", one_call), ("baseline", baseline)) if a.only in (None, w[0])]
        wall = {w: [] for w, _ in ways}
        events = []
        for p in range(a.passes + 1):                                # pass 0 warms up (and grows the arenas)
            for w, call in ways:
                d_out.zero_()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                res = call()
                e1.record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                check(res)
                if p:
                    wall[w].append((t1 - t0) * 1e3)
                    if w == "one_call":
                        events.append(e0.elapsed_time(e1))
        res = {"fixture": a.fixture, "blocks": n, "symbols": len(raw), "winner": win, "baseline_lib": a.baseline_lib or "this build"}
        for w, _ in ways:
            res["ms_" + w] = round(float(np.median(wall[w])), 3)
            res["ms_all_" + w] = [round(x, 3) for x in wall[w]]
        if events:
            res["ms_one_call_events"] = round(float(np.median(events)), 3)
            res["one_call_GBps"] = round(n * len(raw) / res["ms_one_call"] / 1e6, 3)
        if len(ways) == 2:
            res["one_call_over_baseline"] = round(res["ms_one_call"] / res["ms_baseline"], 4)
        print(json.dumps(res), flush=True)
        del d_in, d_out, d_out4
    dc.set_fqz_limits(0, 0)


if __name__ == "__main__":
    main()
