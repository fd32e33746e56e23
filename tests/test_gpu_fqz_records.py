"""fqzcomp_qual decoding on the device at the scale of a slice (htscodecs_amd/csrc/r4x16_fqz.hip): the reference-made
streams of tests/golden/fqzcomp/records.bin - thousands of records, so that the `len`, `sel`, `revcomp` and `dup` models
halve, the two-entry models in registers swap at a halving, and the end pass under GFLAG_DO_REV takes a second trip of
64 records and more - and the batch: total_out_size past k_fq_plan's first trip of 64 blocks and across chunks, the
stage arena without room for a stream's parameter blocks, a host batch in which some streams are refused.

Bytes, lengths, record counts, statuses and routes are the Python model's (fqz_model.py), which test_fqz_cpu.py pins to
the reference on the same file; everything is exact.  Every device call runs in the confinement layout of
fqz_gpu.run_dev."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import fqz_model as M
from fqz_gpu import answer, check, run_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dc():
    import htscodecs_amd as H
    return H.DeviceCodec(0)


@pytest.fixture(scope="module")
def vec():
    """records.bin's inputs by name: (name, data or None, lens, flags, stream, size, SHA-256 or None)"""
    return {i[0]: i for i in M.records()[0]}


def same_as_input(out, inp):
    name, data, lens, flags, stream, size, digest = inp
    return len(out) == size and (out == data if data is not None else hashlib.sha256(out).digest() == digest)


# ---- the vectors -----------------------------------------------------------------------------------------------------
def test_every_input_of_records_bin_in_one_batch(dc):
    inputs, _ = M.records()
    outs, st, lens, nrec, route = check(dc, [i[4] for i in inputs])
    assert st == [0] * len(inputs)
    for inp, out, got in zip(inputs, outs, lens):
        assert same_as_input(out, inp) and got == inp[2], inp[0]
    assert route["streams"] == route["tab_lds"] == route["do_rev"] == len(inputs) and route["multi_param"] == 1
    assert route["dup"] >= 3                                         # records, bit_swap, dup_long


@pytest.mark.parametrize("name", ["records", "rev_trips", "rev_edges", "bit_swap", "dup_long"])
def test_each_input_of_records_bin_alone(dc, vec, name):
    outs, st, lens, nrec, route = check(dc, [vec[name][4]])
    assert st == [0] and same_as_input(outs[0], vec[name]) and lens == [vec[name][2]] and nrec == [len(vec[name][2])]
    assert route["streams"] == 1


def test_records_under_lengths_slots_of_0_1_64_exact_and_roomy(dc, vec):
    stream, want = vec["records"][4], vec["records"][2]
    caps = [0, 1, 64, len(want), len(want) + 5]
    outs, st, lens, nrec, route = check(dc, [stream] * len(caps), len_caps=caps)
    assert st == [0] * len(caps) and nrec == [len(want)] * len(caps)
    assert lens == [want[:c] for c in caps] and all(same_as_input(o, vec["records"]) for o in outs)


def test_the_damaged_variants_of_records_against_the_references_answers(dc):
    _, damaged = M.records()
    outs, st, lens, nrec, route = check(dc, [s for s, _ in damaged])
    for i, (stream, ans) in enumerate(damaged):
        if ans is None:
            assert st[i] != 0, i
        else:
            assert st[i] == 0 and (len(outs[i]), nrec[i], hashlib.sha256(outs[i]).hexdigest()) == ans, i
    assert route["streams"] == len(damaged)                          # the header is whole: every one reaches a wave


def test_records_and_rev_trips_through_the_host_calls(dc, vec):
    import htscodecs_amd as H
    both = [vec["records"], vec["rev_trips"]]
    texts = [answer(i[4])[1] for i in both]
    assert all(same_as_input(t, i) for t, i in zip(texts, both))
    res, st, lens, nrec = H.fqz_uncompress_batch([i[4] for i in both], nlengths=[len(i[2]) for i in both])
    assert (res, st, lens, nrec) == (texts, [0, 0], [i[2] for i in both], [len(i[2]) for i in both])
    for inp, text in zip(both, texts):
        stream, want = inp[4], inp[2]
        assert H.fqz_decompress(stream, nlengths=len(want)) == (text, want)
        assert H.fqz_decompress(stream, nlengths=65) == (text, want[:65])
        # the reference's `lengths[rec] = len` for rec < nlengths: the entries behind the last record stay as they were
        assert H.fqz_decompress(stream, nlengths=len(want) + 3) == (text, want + [-1, -1, -1])


# ---- a wave's second stream after halved models ----------------------------------------------------------------------
def test_one_slot_decodes_four_streams_whose_record_models_halved(dc, vec):
    """one wave takes all four: the `len` and `sel` models in LDS, the `revcomp` and `dup` entries in registers and the
    record table of the stream before are halved, swapped and thousands of records long when the next one starts"""
    order = ["records", "bit_swap", "records", "rev_trips"]
    dc.set_fqz_limits(max_slots=1)
    try:
        outs, st, lens, nrec, route = check(dc, [vec[k][4] for k in order])
    finally:
        dc.set_fqz_limits()
    assert st == [0] * 4 and lens == [vec[k][2] for k in order]
    assert all(same_as_input(o, vec[k]) for o, k in zip(outs, order))


# ---- total_out_size ----------------------------------------------------------------------------------------------------
def planned(streams, caps, total):
    """the header's rule, block by block in their order: a block that the walk accepts adds its stored size to the sum,
    and one that finds the sum above the total is UNSUPPORTED - its claim stays taken.  -> ([(status, bytes or None)],
    the streams that reach a wave)"""
    res, waves, run = [], 0, 0
    for s, cap in zip(streams, caps):
        st, h = M.parse(s)
        if st == 0 and cap < h.out_size:
            st = M.E_CAPACITY
        if st != 0:
            res.append((st, None))
            continue
        run += h.out_size
        if run > total:
            res.append((M.E_UNSUPPORTED, None))
            continue
        st, out, _, _ = answer(s)                                    # (a stream refused inside the loop has reached its wave)
        res.append((st, out if st == 0 else None))
        waves += h.out_size > 0
    return res, waves


def refused_streams(max_sym):
    """[header-refused], [refused inside the loop: x >= nparam, len against the remainder, a duplicate too long]"""
    head = [s for s, site in M.model_refused() if site in ("short", "version", "nparam", "qmap")] + M.model_undefined()[:2]
    loop, sites = [], {}
    for s, ans in M.edge()[1]:
        st, h = M.parse(s)
        if ans is not None or st != 0 or not 0 < h.out_size <= 1200 or h.max_sym > max_sym:
            continue
        ev = []
        M.decompress(s, events=ev)
        site = next(e for e in ev if e.startswith("refuse:"))
        if sites.setdefault(site, 0) < 3:
            sites[site] += 1
            loop.append(s)
    assert sites.get("refuse:len_remainder") == 3 and sites.get("refuse:param") == 3 and sites.get("refuse:dup_length") == 3, sites
    return head, loop


def test_total_out_size_runs_out_at_blocks_63_64_65_127_128_and_the_last(dc):
    good = [i[4] for i in M.edge()[0] if 0 < i[5] <= 1200]
    max_sym = max(M.parse(s)[1].max_sym for s in good)
    head, loop = refused_streams(max_sym)
    n, at = 150, (63, 64, 65, 127, 128, 149)
    bad = head + loop
    streams, g, b = [], 0, 0
    for k in range(n):
        if k % 5 == 3 and k not in at:                               # (a good stream at every index a total runs out at)
            streams.append(bad[b % len(bad)])
            b += 1
        else:
            streams.append(good[g % len(good)])
            g += 1
    assert b >= len(bad) and g > 2 * len(good)
    sizes = [M.parse(s)[1].out_size if M.parse(s)[0] == 0 else 0 for s in streams]
    assert all(z > 0 for s, z in zip(streams, sizes) if M.parse(s)[0] == 0)      # no stored size of 0 behind a crossing
    caps = [max(z, 1) for z in sizes]
    assert sum(M.parse(s)[1].nparam for s in streams if M.parse(s)[0] == 0) <= 4 * n     # the arena has room for all
    dc.set_fqz_limits(max_sym=max_sym)
    try:
        for first in at + (None,):
            total = sum(sizes) if first is None else sum(sizes[:first + 1]) - 1
            want, waves = planned(streams, caps, total)
            outs, st, _, nrec, route = run_dev(dc, streams, caps, total=total, want_chunks=1)
            assert st == [w[0] for w in want], (first, [(k, a, w[0]) for k, (a, w) in enumerate(zip(st, want)) if a != w[0]][:8])
            assert outs == [w[1] for w in want], first
            assert route["streams"] == waves, (first, route, waves)
            refused = [k for k in range(n) if st[k] == M.E_UNSUPPORTED and M.parse(streams[k])[0] == 0]
            if first is None:
                assert not refused and waves == sum(M.parse(s)[0] == 0 for s in streams)      # the exact total: all decode
            else:
                assert refused[0] == first and refused == [k for k in range(first, n) if M.parse(streams[k])[0] == 0]
    finally:
        dc.set_fqz_limits()


def test_total_out_size_runs_out_in_the_second_and_third_chunk(dc):
    fx = M.fixtures()
    streams = [fx[k][2] for k in (12, 13, 14, 15)] + [i[4] for i in M.edge()[0][:4]]
    sizes = [M.parse(s)[1].out_size for s in streams]
    assert all(z > 0 for z in sizes)
    was = dc.get_option("max_workspace_mb")
    dc.set_fqz_limits(max_sym=50)                                    # a slot: 65,536 x (4 x 52 + 4) bytes = 13.25 MiB
    dc.set_option("max_workspace_mb", 48)                            # three slots and the stage arena: chunks of 3, 3, 2
    try:
        for first in (3, 5, 6):                                      # the first of the second chunk, its last, the first of the third
            total = sum(sizes[:first + 1]) - 1
            want, waves = planned(streams, sizes, total)
            assert [w[0] for w in want] == [0] * first + [M.E_UNSUPPORTED] * (8 - first) and waves == first
            outs, st, _, nrec, route = run_dev(dc, streams, sizes, total=total, want_chunks=3)
            assert st == [w[0] for w in want], (first, st)
            assert outs == [w[1] for w in want], first
            assert route["streams"] == waves, (first, route)
    finally:
        dc.set_option("max_workspace_mb", was)
        dc.set_fqz_limits()


# ---- no room for a stream's parameter blocks ----------------------------------------------------------------------------
def test_copies_of_a_nine_block_stream_beyond_the_arenas_room_are_refused_whole(dc):
    """The stage arena holds four parameter blocks a block of the chunk: of n streams with nine each, some find no room.
    Which ones is the order in which the waves of k_fq_front claim their place, so only the contract is asserted."""
    stream = next(i[4] for i in M.edge()[0] if i[0] == "nparam9")
    h = M.parse(stream)[1]
    text = answer(stream)[1]
    assert h.nparam == 9 and answer(stream)[0] == 0 and len(text) == h.out_size
    dc.set_fqz_limits(max_sym=h.max_sym)
    try:
        for n in (96, 128, 192, 256):
            outs, st, lens, nrec, route = run_dev(dc, [stream] * n, [h.out_size] * n, len_caps=[len(answer(stream)[2])] * n,
                                                  total=n * h.out_size, want_chunks=1)      # (run_dev: nothing outside the slots)
            if any(st):
                break
        accepted = [k for k in range(n) if st[k] == 0]
        assert len(accepted) < n, "no copy was refused up to 256"
        assert len(accepted) >= max(4 * n, 256) // 9, (n, len(accepted))
        for k in range(n):
            if st[k] == 0:
                assert outs[k] == text and lens[k] == answer(stream)[2] and nrec[k] == len(lens[k]), k
            else:
                assert st[k] == M.E_UNSUPPORTED and outs[k] is None and nrec[k] == 0, (k, st[k])     # (run_dev: size 0)
        assert route["streams"] == route["tab_global"] == len(accepted), (route, len(accepted))
        outs, st, _, _, route = check(dc, [stream] * 20)             # the same context, a fresh call: the arena starts empty
        assert st == [0] * 20 and route["streams"] == 20
    finally:
        dc.set_fqz_limits()


# ---- a host batch in which streams are refused --------------------------------------------------------------------------
def host_batch(ctx, blocks, caps, nlengths):
    """rans4x16_hip_fqz_uncompress_batch as it is: -> (return value, statuses, sizes, output buffers, lengths arrays, nrec)"""
    n = len(blocks)
    srcs = [np.frombuffer(bytes(b) or b"\0", dtype=np.uint8) for b in blocks]
    outs = [np.full(max(c, 1), 0xa5, dtype=np.uint8) for c in caps]
    lens = [np.full(max(v, 1), -1, dtype=np.int32) for v in nlengths]
    in_p = (C.c_void_p * n)(*[s.ctypes.data for s in srcs])
    out_p = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    len_p = (C.c_void_p * n)(*[a.ctypes.data for a in lens])
    in_sz = (C.c_uint * n)(*[len(b) for b in blocks])
    out_sz = (C.c_uint * n)(*caps)
    nl = (C.c_int * n)(*nlengths)
    nrec = (C.c_uint * n)(*([77] * n))
    status = (C.c_int * n)(*([-7] * n))
    rc = ctx.L.rans4x16_hip_fqz_uncompress_batch(ctx.h, n, in_p, in_sz, out_p, out_sz, status, len_p, nl, nrec)
    return rc, list(status), list(out_sz), outs, lens, list(nrec)


def test_a_host_batch_of_refused_and_accepted_streams(vec):
    import htscodecs_amd as H
    edge_in = {i[0]: i[4] for i in M.edge()[0]}
    version = next(s for s, site in M.model_refused() if site == "version")
    remainder = None
    for s, ans in M.edge()[1]:
        ev = []
        if ans is None and M.parse(s)[0] == 0 and M.decompress(s, events=ev)[0] != 0 and "refuse:len_remainder" in ev:
            remainder = s
            break
    blocks = [b"", version, M.model_undefined()[2], remainder, edge_in["empty"], edge_in["nparam3"], edge_in["rev"], edge_in["starts"],
              vec["records"][4]]
    stored = [M.parse(s)[1].out_size if s else 0 for s in blocks]
    caps = list(stored)
    caps[6] -= 1                                                     # `rev`: one byte short
    caps[0] = caps[1] = 8
    nrecs = [len(answer(s)[2]) if s else 0 for s in blocks]
    nlengths = [3, 0, 1, 5, 2, nrecs[5], 4, nrecs[7] + 3, nrecs[8] + 3]      # 0, 1, exact and + 3 among them
    want = []
    for s, cap in zip(blocks, caps):
        st, out, lens, _ = answer(s) if s else (M.E_EMPTY, b"", [], None)
        if M.parse(s)[0] == 0 and cap < M.parse(s)[1].out_size:
            st, out, lens = M.E_CAPACITY, b"", []
        want.append((st, out, lens))
    assert [w[0] for w in want] == [M.E_EMPTY, M.E_UNSUPPORTED, M.E_TABLE, M.E_SIZE, 0, 0, M.E_CAPACITY, 0, 0]
    ctx = H.codec._thread_ctx()
    rc, st, sizes, outs, lens, nrec = host_batch(ctx, blocks, caps, nlengths)
    assert st == [w[0] for w in want], st
    assert rc == sum(s != 0 for s in st) == 5
    for k, (wst, wout, wlens) in enumerate(want):
        if wst:
            assert sizes[k] == 0 and nrec[k] == 0 and (lens[k] == -1).all(), k
        else:
            assert sizes[k] == len(wout) and outs[k][:sizes[k]].tobytes() == wout and nrec[k] == len(wlens), k
            got = min(nlengths[k], len(wlens))
            assert lens[k][:got].tolist() == wlens[:got] and (lens[k][got:] == -1).all(), k
    assert same_as_input(outs[8][:sizes[8]].tobytes(), vec["records"]) and nrec[8] == len(vec["records"][2])
    # the wrapper over the same batch
    res, st2, lens2, nrec2 = H.fqz_uncompress_batch(blocks, caps=caps, nlengths=nlengths)
    assert st2 == st and nrec2 == nrec
    assert res == [w[1] if w[0] == 0 else None for w in want]
    assert lens2 == [w[2][:nl] for w, nl in zip(want, nlengths)]
