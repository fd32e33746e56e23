#!/usr/bin/env python3
"""Rate of rans4x16_hip_arith_compress_dev (include/rans4x16_hip.h part 2h): HIP events around the device call after a
warm-up pass, several passes, the median taken; GB/s of input bytes.  One JSON line per shape and batch size.

Shapes, those of tools/arith_rate.py: 1 MiB blocks of q40 text under order 0 and order 1 (rows in LDS), the same text with
100 added to every byte under order 1 (an alphabet above the LDS budget: rows in global memory), q4 text under order 64
(run lengths).  A batch is ONE block repeated: the blocks of a batch are independent of each other.  Every pass's output
is decoded again on the device (rans4x16_hip_arith_uncompress_dev) and compared with the input, and every block's stream
with the first block's."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("o0_q40", "q40+dir", 0, 0), ("o1_q40_lds", "q40+dir", 1, 0), ("o1_q40_global", "q40+dir", 1, 100), ("o0_rle_q4", "q4", 64, 0))


def text(name, size, shift):
    t = np.fromfile(os.path.join(ROOT, "tests", "golden", "dat", name + ".nl"), dtype=np.uint8)
    return ((np.resize(t, size).astype(np.uint16) + shift) & 0xff).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1 << 20)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=[k for k, _, _, _ in SHAPES])
    a = ap.parse_args()
    import torch
    import htscodecs_amd as H
    from htscodecs_amd import codec
    assert torch.cuda.is_available(), "arith_enc_rate.py measures on a GPU"
    dc = H.DeviceCodec(0)
    dc.set_option("route_count", 1)
    for key, name, order, shift in SHAPES:
        if key not in a.shapes:
            continue
        raw = text(name, a.size, shift)
        cap = codec.arith_compress_cap(a.size, order)
        for n in a.batches:
            stride_in, stride_out = (a.size + 255) // 256 * 256, (cap + 255) // 256 * 256
            d_raw = torch.from_numpy(raw).to(dc.dev)
            d_in = torch.zeros(n * stride_in + 64, dtype=torch.uint8, device=dc.dev)
            d_in[:n * stride_in].view(n, stride_in)[:, :a.size] = d_raw
            d_out = torch.zeros(n * stride_out + 64, dtype=torch.uint8, device=dc.dev)
            d_back = torch.zeros(n * stride_in, dtype=torch.uint8, device=dc.dev)
            i64 = lambda v: torch.arange(n, dtype=torch.int64, device=dc.dev) * v
            i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dc.dev)
            d_osz, d_st, d_bsz, d_bst = i32(-1), i32(-1), i32(-1), i32(-1)
            d_isz, d_cap = i32(a.size), i32(cap)
            in_off, out_off = i64(stride_in), i64(stride_out)
            ms, dec_ms, coded = [], [], 0
            dc.route_read("arith_enc")
            for p in range(a.passes + 1):                            # pass 0 warms up
                d_out.zero_()
                d_back.zero_()
                e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
                e0.record()
                dc.arith_compress(d_in, in_off, d_isz, d_out, out_off, d_cap, d_osz, d_st, order, a.size,
                                  total_in_size=n * a.size)
                e1.record()
                torch.cuda.synchronize()
                assert d_st.eq(0).all().item(), key
                coded = int(d_osz[0].item())
                assert d_osz.eq(coded).all().item() and coded < a.size, key
                assert d_out[:n * stride_out].view(n, stride_out)[:, :coded].eq(d_out[:coded]).all().item(), key + ": the blocks' streams differ"
                e2.record()
                dc.arith_uncompress(d_out, out_off, d_osz, d_back, in_off, d_isz, d_bsz, d_bst, coded, a.size, n * a.size)
                e3.record()
                torch.cuda.synchronize()
                assert d_bst.eq(0).all().item() and d_bsz.eq(a.size).all().item(), key
                assert d_back.view(n, stride_in)[:, :a.size].eq(d_raw).all().item(), key + ": the streams do not decode to the input"
                if p:
                    ms.append(e0.elapsed_time(e1))
                    dec_ms.append(e2.elapsed_time(e3))
            route = {k: v // (a.passes + 1) for k, v in dc.route_read("arith_enc").items() if v}
            med, dmed = float(np.median(ms)), float(np.median(dec_ms))
            print(json.dumps({"shape": key, "order": order, "blocks": n, "block_bytes": a.size, "stream_bytes": coded,
                              "ms_median": round(med, 3), "ms_all": [round(x, 3) for x in ms],
                              "GBps_input": round(n * a.size / med / 1e6, 3),
                              "decode_ms_median": round(dmed, 3), "route_per_pass": route}), flush=True)
            del d_in, d_out, d_back


if __name__ == "__main__":
    main()
