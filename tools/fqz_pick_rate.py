#!/usr/bin/env python3
"""Rate of the device pick (include/rans4x16_hip.h part 2k), beside tools/fqz_enc_rate.py and with its method: HIP events
around the device call after a warm-up pass, five passes, the median taken, every pass's output compared with the
reference's.  One JSON line per shape.

Per fixture (default q40+dir.0 and q4.0) and batch size (1, 256, 1,024 blocks of the fixture's text, the blocks
independent): rans4x16_hip_fqz_pick_dev alone, rans4x16_hip_fqz_compress_pick_dev, and as the yardstick of the same run
rans4x16_hip_fqz_compress_dev with the parameter bytes given (the chain).  Then the host pick on one and on eight threads
(rans4x16_hip_fqz_pick_parameters; wall clock), and the host-buffer batch with params NULL under
rans4x16_hip_set_fqz_pick mode 0 and mode 1 at 64 and 1,024 blocks (wall clock)."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixtures", nargs="+", default=["q40+dir.0", "q4.0"])
    ap.add_argument("--blocks", type=int, nargs="+", default=[1, 256, 1024])
    ap.add_argument("--host-blocks", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    import torch
    import fqz_enc_model as E
    import htscodecs_amd as H
    assert torch.cuda.is_available(), "fqz_pick_rate.py measures on a GPU"
    dc = H.DeviceCodec(0)
    dev = dc.dev
    pcap = H.fqz_pick_cap()
    for fixture in a.fixtures:
        fn, strat, stream, raw, lens, flags = next(f for f in E.fixture_slices() if f[0] == fixture)
        st, par, lens2, flags2 = H.fqz_pick_parameters(raw, lens, flags, 4, strat)
        assert st == 0 and par == E.params_of(stream)
        dc.set_fqz_limits(max_sym=H.fqz_scan(stream)[1]["max_sym"])
        cap = H.fqz_compress_cap(len(raw), len(lens), pcap)
        up = lambda arr: torch.from_numpy(np.asarray(arr, dtype=np.int64).astype(np.uint32).view(np.int32).copy()).to(dev)
        u8 = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(dev)
        for n in a.blocks:
            stride_in, stride_out, nrec = (len(raw) + 255) // 256 * 256, (cap + 255) // 256 * 256, len(lens)
            d_in = torch.zeros(n * stride_in + 64, dtype=torch.uint8, device=dev)
            d_in[:n * stride_in].view(n, stride_in)[:, :len(raw)] = u8(raw)
            d_out = torch.zeros(n * stride_out, dtype=torch.uint8, device=dev)
            d_par = torch.zeros(n * pcap, dtype=torch.uint8, device=dev)
            d_len, d_fl = up(lens * n), up(flags * n)                # every block its own records: the pick writes them back
            d_lo, d_fo = torch.zeros_like(d_len), torch.zeros_like(d_fl)
            d_len2, d_fl2, d_par1 = up(lens2), up(flags2), u8(par)
            i64 = lambda v: torch.arange(n, dtype=torch.int64, device=dev) * v
            i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)
            d_osz, d_st = i32(-1), i32(-1)
            want, want_par = u8(stream), u8(par)
            want_fl = up(flags2)

            def pick():
                dc.fqz_pick(d_in, i64(stride_in), i32(len(raw)), d_len, d_fl, i64(nrec), i32(nrec), d_par, i64(pcap), i32(pcap), d_osz,
                            d_lo, d_fo, d_st, len(raw), nrec, vers=4, strat=strat)

            def pick_ok():
                assert d_st.eq(0).all().item() and d_osz.eq(len(par)).all().item()
                assert d_par.view(n, pcap)[:, :len(par)].eq(want_par).all().item() and d_fo.view(n, nrec).eq(want_fl).all().item()

            def one_call():
                dc.fqz_compress_pick(d_in, i64(stride_in), i32(len(raw)), d_len, d_fl, i64(nrec), i32(nrec), d_out, i64(stride_out), i32(cap),
                                     d_osz, d_st, len(raw), nrec, vers=4, strat=strat)

            def chain():
                dc.fqz_compress(d_in, i64(stride_in), i32(len(raw)), d_par1, i64(0), i32(len(par)), d_len2, d_fl2, i64(0), i32(nrec),
                                d_out, i64(stride_out), i32(cap), d_osz, d_st, len(raw), len(par), nrec)

            def stream_ok():
                assert d_st.eq(0).all().item() and d_osz.eq(len(stream)).all().item()
                assert d_out.view(n, stride_out)[:, :len(stream)].eq(want).all().item(), "bytes differ"

            res = {"shape": "device", "fixture": fn, "blocks": n, "symbols": len(raw)}
            for what, call, ok in (("pick", pick, pick_ok), ("compress_pick", one_call, stream_ok), ("chain_params_given", chain, stream_ok)):
                ms = []
                for p in range(a.passes + 1):                        # pass 0 warms up (and grows the arena)
                    d_out.zero_(); d_par.zero_()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call()
                    e1.record()
                    torch.cuda.synchronize()
                    ok()
                    if p:
                        ms.append(e0.elapsed_time(e1))
                res["ms_" + what] = round(float(np.median(ms)), 3)
                res["ms_all_" + what] = [round(x, 3) for x in ms]
            res["pick_GBps"] = round(n * len(raw) / res["ms_pick"] / 1e6, 3)
            res["pick_share_of_one_call"] = round(res["ms_pick"] / res["ms_compress_pick"], 3)
            print(json.dumps(res), flush=True)
            del d_in, d_out, d_par
        # the host pick, one thread and eight (the library's pick releases the GIL inside the C call)
        n = max(a.blocks)
        one = lambda _: H.fqz_pick_parameters(raw, lens, flags, 4, strat)[0]
        res = {"shape": "host_pick", "fixture": fn, "blocks": n}
        for threads in (1, 8):
            t0 = time.perf_counter()
            with ThreadPoolExecutor(threads) as ex:
                assert not any(ex.map(one, range(n)))
            res["ms_%d_threads" % threads] = round((time.perf_counter() - t0) * 1e3, 1)
        res["MBps_one_thread"] = round(n * len(raw) / res["ms_1_threads"] / 1e3, 1)
        print(json.dumps(res), flush=True)
        for n in a.host_blocks:
            res = {"shape": "host_batch", "fixture": fn, "blocks": n}
            for mode in (0, 1):
                dc.set_fqz_pick(mode, 0)
                wall = []
                for p in range(a.passes + 1):
                    t0 = time.perf_counter()
                    outs, sts, _, _ = H.fqz_compress_batch([raw] * n, [lens] * n, [flags] * n, 4, strat, ctx=dc.ctx)
                    t1 = time.perf_counter()
                    assert sts == [0] * n and all(o == stream for o in outs), mode
                    if p:
                        wall.append((t1 - t0) * 1e3)
                res["ms_mode_%d" % mode] = round(float(np.median(wall)), 1)
            dc.set_fqz_pick(0, 0)
            print(json.dumps(res), flush=True)
        dc.set_fqz_limits(0, 0)


if __name__ == "__main__":
    main()
