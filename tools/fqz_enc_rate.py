#!/usr/bin/env python3
"""Rate of rans4x16_hip_fqz_compress_dev (include/rans4x16_hip.h part 2j), beside tools/fqz_rate.py for the decoder: HIP
events around the device call after a warm-up pass, several passes, the median taken.  One JSON line per shape:
nanoseconds per symbol for one stream alone, and GB/s of encoded input at 1, 4 and 16 streams per compute unit.

The block is the text of a reference-made fixture (tests/golden/fqzcomp, default q40+dir.0: 100,000 qualities in 1,000
records) under the parameters the host pick chooses for it, repeated: the blocks of a batch are independent.  The model
slots are sized for the parameters' max_sym (rans4x16_hip_set_fqz_limits).  Every pass's output is compared with the
reference's stream - the same streams tools/fqz_rate.py decodes.

--host N: the host-buffer batch instead (rans4x16_hip_fqz_compress_batch over N such blocks), wall clock: with params
NULL (every block picked on the host first), with the parameter bytes given, and the pick alone (one thread, through
rans4x16_hip_fqz_pick_parameters)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default="q40+dir.0")
    ap.add_argument("--per-cu", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--host", type=int, default=0)
    a = ap.parse_args()
    import torch
    import fqz_enc_model as E
    import htscodecs_amd as H
    assert torch.cuda.is_available(), "fqz_enc_rate.py measures on a GPU"
    fn, strat, stream, raw, lens, flags = next(f for f in E.fixture_slices() if f[0] == a.fixture)
    st, par, lens2, flags2 = H.fqz_pick_parameters(raw, lens, flags, 4, strat)
    assert st == 0
    info = H.fqz_scan(stream)[1]
    if a.host:
        n = a.host
        res = {"shape": "host_batch", "fixture": fn, "blocks": n, "symbols": len(raw), "pick_threads": min(n, os.cpu_count() or 1, 8)}
        for what, params in (("picked", None), ("given", [par] * n)):
            best = []
            for p in range(a.passes + 1):
                t0 = time.perf_counter()
                outs, sts, _, _ = H.fqz_compress_batch([raw] * n, [lens2 if params else lens] * n, [flags2 if params else flags] * n, 4, strat, params=params)
                t1 = time.perf_counter()
                assert sts == [0] * n and all(o == stream for o in outs), what
                if p:
                    best.append((t1 - t0) * 1e3)
            res["ms_" + what] = round(float(np.median(best)), 2)
        t0 = time.perf_counter()
        for _ in range(n):
            assert H.fqz_pick_parameters(raw, lens, flags, 4, strat)[0] == 0
        res["ms_pick_alone_one_thread"] = round((time.perf_counter() - t0) * 1e3, 2)
        res["pick_MBps_one_thread"] = round(n * len(raw) / res["ms_pick_alone_one_thread"] / 1e3, 1)
        res["pick_share_of_batch"] = round(max(res["ms_picked"] - res["ms_given"], 0.0) / res["ms_picked"], 3)
        print(json.dumps(res), flush=True)
        return
    dc = H.DeviceCodec(0)
    dc.set_option("route_count", 1)
    dc.set_fqz_limits(max_sym=info["max_sym"])
    cus = torch.cuda.get_device_properties(dc.dev).multi_processor_count
    cap = H.fqz_compress_cap(len(raw), len(lens2), len(par))
    up = lambda arr: torch.from_numpy(np.asarray(arr, dtype=np.int64).astype(np.uint32).view(np.int32).copy()).to(dc.dev)
    for what, n in [("alone", 1)] + [("%d_per_cu" % k, k * cus) for k in a.per_cu]:
        stride_in, stride_out = (len(raw) + 255) // 256 * 256, (cap + 255) // 256 * 256
        d_in = torch.zeros(n * stride_in + 64, dtype=torch.uint8, device=dc.dev)
        d_in[:n * stride_in].view(n, stride_in)[:, :len(raw)] = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dc.dev)
        d_out = torch.zeros(n * stride_out, dtype=torch.uint8, device=dc.dev)
        d_par = torch.from_numpy(np.frombuffer(par, dtype=np.uint8).copy()).to(dc.dev)
        d_len, d_fl = up(lens2), up(flags2)
        i64 = lambda v: torch.arange(n, dtype=torch.int64, device=dc.dev) * v
        i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dc.dev)
        d_osz, d_st = i32(-1), i32(-1)
        want = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).to(dc.dev)
        ms = []
        dc.route_read("fqz_enc")
        for p in range(a.passes + 1):                                # pass 0 warms up (and grows the arena)
            d_out.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dc.fqz_compress(d_in, i64(stride_in), i32(len(raw)), d_par, i64(0), i32(len(par)), d_len, d_fl, i64(0), i32(len(lens2)),
                            d_out, i64(stride_out), i32(cap), d_osz, d_st, len(raw), len(par), len(lens2))
            e1.record()
            torch.cuda.synchronize()
            assert d_st.eq(0).all().item() and d_osz.eq(len(stream)).all().item(), what
            assert d_out.view(n, stride_out)[:, :len(stream)].eq(want).all().item(), what + ": bytes differ"
            if p:
                ms.append(e0.elapsed_time(e1))
        route = {k: v // (a.passes + 1) for k, v in dc.route_read("fqz_enc").items() if v}
        med = float(np.median(ms))
        waves = min(n, 1024)
        print(json.dumps({"shape": what, "fixture": fn, "blocks": n, "symbols": len(raw), "stream_bytes": len(stream), "max_sym": info["max_sym"],
                          "ms_median": round(med, 3), "ms_all": [round(x, 3) for x in ms],
                          "ns_per_symbol_per_wave": round(med * 1e6 / (len(raw) * -(-n // waves)), 1),
                          "GBps_encoded": round(n * len(raw) / med / 1e6, 4),
                          "route_per_pass": route}), flush=True)
        del d_in, d_out


if __name__ == "__main__":
    main()
