#!/usr/bin/env python3
"""Rate of rans4x16_hip_arith_uncompress_dev (include/rans4x16_hip.h part 2g): HIP events around the device call after a
warm-up pass, several passes, the median taken; GB/s of decoded bytes.  One JSON line per shape.

Shapes: 1 MiB blocks of q40 text under order 0 and order 1 (rows in LDS), the same text with 100 added to every byte under
order 1 (an alphabet above the LDS budget: rows in global memory), q4 text under order 64 (run lengths), each at two
batch sizes.  A batch is ONE stream repeated: the streams of a batch are independent, so their content does not matter
to the rate, and the Python coder that makes them (tests/arith_model.py) takes seconds per MiB.  --streams FILE keeps
the coded streams between runs (numpy .npz).  Every pass's output is compared with the raw text."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = (("o0_q40", "q40+dir", 0, 0), ("o1_q40_lds", "q40+dir", 1, 0), ("o1_q40_global", "q40+dir", 1, 100), ("o0_rle_q4", "q4", 64, 0))


def make_streams(size, path):
    import arith_model as M
    if path and os.path.exists(path):
        z = np.load(path)
        if int(z["size"]) == size:
            return {k: (z[k + "_raw"].tobytes(), z[k + "_stream"].tobytes()) for k, _, _, _ in SHAPES}
    out = {}
    for key, name, order, shift in SHAPES:
        t = np.frombuffer(M.text(name), dtype=np.uint8)
        raw = ((np.resize(t, size).astype(np.uint16) + shift) & 0xff).astype(np.uint8).tobytes()
        out[key] = (raw, M.compress(raw, order))
    if path:
        np.savez(path, size=size, **{k + "_raw": np.frombuffer(v[0], dtype=np.uint8) for k, v in out.items()},
                 **{k + "_stream": np.frombuffer(v[1], dtype=np.uint8) for k, v in out.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1 << 20)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--streams", default=None)
    ap.add_argument("--shapes", nargs="+", default=[k for k, _, _, _ in SHAPES])
    ap.add_argument("--make-only", action="store_true", help="code the streams into --streams and stop (needs no GPU)")
    a = ap.parse_args()
    streams = make_streams(a.size, a.streams)
    if a.make_only:
        return
    import torch
    import htscodecs_amd as H
    assert torch.cuda.is_available(), "arith_rate.py measures on a GPU"
    dc = H.DeviceCodec(0)
    dc.set_option("route_count", 1)
    for key, _, order, _ in SHAPES:
        if key not in a.shapes:
            continue
        raw, s = streams[key]
        for n in a.batches:
            stride_in, stride_out = (len(s) + 255) // 256 * 256, (len(raw) + 255) // 256 * 256
            d_in = torch.zeros(n * stride_in + 64, dtype=torch.uint8, device=dc.dev)
            d_in[:n * stride_in].view(n, stride_in)[:, :len(s)] = torch.from_numpy(np.frombuffer(s, dtype=np.uint8).copy()).to(dc.dev)
            d_out = torch.zeros(n * stride_out, dtype=torch.uint8, device=dc.dev)
            i64 = lambda v: torch.arange(n, dtype=torch.int64, device=dc.dev) * v
            i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dc.dev)
            d_osz, d_st = i32(-1), i32(-1)
            args = (d_in, i64(stride_in), i32(len(s)), d_out, i64(stride_out), i32(len(raw)), d_osz, d_st, len(s), len(raw), n * len(raw))
            want = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dc.dev)
            ms = []
            dc.route_read("arith")
            for p in range(a.passes + 1):                            # pass 0 warms up
                d_out.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dc.arith_uncompress(*args)
                e1.record()
                torch.cuda.synchronize()
                assert d_st.eq(0).all().item() and d_osz.eq(len(raw)).all().item(), key
                assert d_out.view(n, stride_out)[:, :len(raw)].eq(want).all().item(), key + ": bytes differ"
                if p:
                    ms.append(e0.elapsed_time(e1))
            route = {k: v // (a.passes + 1) for k, v in dc.route_read("arith").items() if v}
            med = float(np.median(ms))
            print(json.dumps({"shape": key, "order": order, "blocks": n, "block_bytes": len(raw), "stream_bytes": len(s),
                              "ms_median": round(med, 3), "ms_all": [round(x, 3) for x in ms],
                              "GBps_decoded": round(n * len(raw) / med / 1e6, 3), "route_per_pass": route}), flush=True)
            del d_in, d_out


if __name__ == "__main__":
    main()
