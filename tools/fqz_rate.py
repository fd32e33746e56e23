#!/usr/bin/env python3
"""Rate of rans4x16_hip_fqz_uncompress_dev (include/rans4x16_hip.h part 2i): HIP events around the device call after a
warm-up pass, several passes, the median taken.  One JSON line per shape: nanoseconds per symbol for one stream alone,
and GB/s of decoded bytes at 1, 4 and 16 streams per compute unit.

The stream is a reference-made fixture (tests/golden/fqzcomp, default q40+dir.0: 100,000 qualities in 1,000 records, one
parameter block, max_sym 44) repeated: the streams of a batch are independent, so their content does not matter to the
rate.  The model slots are sized for the fixture's max_sym (rans4x16_hip_set_fqz_limits); at most 1,024 streams are in
flight, four a compute unit, the others wait for a slot - so 16 streams per compute unit is four streams a wave, one
after the other.  Every pass's output is compared with the text.  Nearest existing kernel for comparison: the order-1
global-home figures of tools/arith_rate.py --shapes o1_q40_global (profiles/arith.md)."""
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
    ap.add_argument("--fixture", default="q40+dir.0")
    ap.add_argument("--per-cu", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    import torch
    import fqz_model as M
    import htscodecs_amd as H
    assert torch.cuda.is_available(), "fqz_rate.py measures on a GPU"
    fn, base, s, raw, lens = next(f for f in M.fixtures() if f[0] == a.fixture)
    st, info = H.fqz_scan(s)
    assert st == 0
    dc = H.DeviceCodec(0)
    dc.set_option("route_count", 1)
    dc.set_fqz_limits(max_sym=info["max_sym"])
    cus = torch.cuda.get_device_properties(dc.dev).multi_processor_count
    for what, n in [("alone", 1)] + [("%d_per_cu" % k, k * cus) for k in a.per_cu]:
        stride_in, stride_out = (len(s) + 255) // 256 * 256, (len(raw) + 255) // 256 * 256
        d_in = torch.zeros(n * stride_in + 64, dtype=torch.uint8, device=dc.dev)
        d_in[:n * stride_in].view(n, stride_in)[:, :len(s)] = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).to(dc.dev)
        d_out = torch.zeros(n * stride_out, dtype=torch.uint8, device=dc.dev)
        i64 = lambda v: torch.arange(n, dtype=torch.int64, device=dc.dev) * v
        i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dc.dev)
        d_osz, d_st, d_nrec = i32(-1), i32(-1), i32(-1)
        want = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dc.dev)
        ms = []
        dc.route_read("fqz")
        for p in range(a.passes + 1):                                # pass 0 warms up (and grows the arena)
            d_out.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dc.fqz_uncompress(d_in, i64(stride_in), i32(len(s)), d_out, i64(stride_out), i32(len(raw)), d_osz, d_st, len(s), len(raw),
                              n * len(raw), nrec=d_nrec)
            e1.record()
            torch.cuda.synchronize()
            assert d_st.eq(0).all().item() and d_osz.eq(len(raw)).all().item() and d_nrec.eq(len(lens)).all().item(), what
            assert d_out.view(n, stride_out)[:, :len(raw)].eq(want).all().item(), what + ": bytes differ"
            if p:
                ms.append(e0.elapsed_time(e1))
        route = {k: v // (a.passes + 1) for k, v in dc.route_read("fqz").items() if v}
        med = float(np.median(ms))
        waves = min(n, 1024)
        print(json.dumps({"shape": what, "fixture": fn, "streams": n, "symbols": len(raw), "stream_bytes": len(s), "max_sym": info["max_sym"],
                          "ms_median": round(med, 3), "ms_all": [round(x, 3) for x in ms],
                          "ns_per_symbol_per_wave": round(med * 1e6 / (len(raw) * -(-n // waves)), 1),
                          "GBps_decoded": round(n * len(raw) / med / 1e6, 4),
                          "route_per_pass": route}), flush=True)
        del d_in, d_out


if __name__ == "__main__":
    main()
