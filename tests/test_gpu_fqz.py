"""fqzcomp_qual decoding on the device (include/rans4x16_hip.h part 2i; htscodecs_amd/csrc/r4x16_fqz.hip): the reference's
16 streams through every entry point, the reference-made inputs and damaged streams of tests/golden/fqzcomp/edge.bin,
the streams the model constructs where the reference is undefined, confinement, a wave's second and third stream, the
walk over chunks, capacity and total_out_size.

Bytes, lengths, record counts, statuses and routes are the Python model's (fqz_model.py), which test_fqz_cpu.py pins to
the reference; for the fixtures the bytes are the committed texts.  Every device call runs in the confinement layout of
fqz_gpu.run_dev."""
import hashlib

import pytest

import fqz_model as M
from fqz_gpu import answer, check, expect, run_dev

pytestmark = pytest.mark.gpu
OTHER_ROUTES = ("encode", "decode", "expand", "result", "names", "arith", "arith_enc")


@pytest.fixture(scope="module")
def dc():
    import htscodecs_amd as H
    return H.DeviceCodec(0)


@pytest.fixture(scope="module")
def fx():
    return M.fixtures()


# ---- the fixtures through every entry point ------------------------------------------------------------------------
def test_the_16_fixtures_in_one_batch_through_the_device_call_and_the_batch_call(dc, fx):
    import htscodecs_amd as H
    streams, texts, lens = [f[2] for f in fx], [f[3] for f in fx], [f[4] for f in fx]
    dc.set_option("route_count", 1)
    try:
        for r in OTHER_ROUTES:
            dc.route_read(r)
        outs, st, got_lens, nrec, route = check(dc, streams, want=texts)
        assert got_lens == lens and nrec == [len(v) for v in lens]
        assert route == {"streams": 16, "tab_lds": 16, "tab_global": 0, "do_rev": 0, "multi_param": 0, "dup": route["dup"]}
        assert route["dup"] <= 4                                     # PFLAG_DO_DEDUP is set in the four qvar streams alone
        dc.set_option("route_count", 1)
        for r in OTHER_ROUTES:                                       # no other route moved
            assert not any(dc.route_read(r).values()), r
    finally:
        dc.set_option("route_count", 0)
    res, st, got_lens, nrec = H.fqz_uncompress_batch(streams, nlengths=[len(v) for v in lens])
    assert st == [0] * 16 and res == texts and got_lens == lens and nrec == [len(v) for v in lens]


@pytest.mark.parametrize("k", range(16))
def test_each_fixture_alone_through_the_three_entry_points(dc, fx, k):
    import htscodecs_amd as H
    fn, base, stream, text, lens = fx[k]
    outs, st, got_lens, nrec, route = check(dc, [stream], want=[text])
    assert got_lens == [lens] and route["streams"] == 1
    res, st, got_lens, nrec = H.fqz_uncompress_batch([stream], nlengths=[len(lens) + 3])
    assert (res, st, got_lens, nrec) == ([text], [0], [lens], [len(lens)])
    assert H.fqz_decompress(stream, nlengths=len(lens)) == (text, lens)
    assert H.fqz_decompress(stream, nlengths=7) == (text, lens[:7])
    assert H.fqz_decompress(stream) == (text, [])


def test_peek_gives_the_stored_sizes(dc, fx):
    import numpy as np
    import torch as t
    streams = [f[2] for f in fx] + [b"", b"\x85", M.edge()[0][-1][4]]
    arena = np.frombuffer(b"".join(streams) + bytes(16), dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(s) for s in streams[:-1]]).astype(np.int64)
    up = lambda a: t.from_numpy(a).to(dc.dev)
    raw, st = (t.full((len(streams),), -7, dtype=t.int32, device=dc.dev) for _ in range(2))
    dc.fqz_peek(up(arena), up(off), up(np.array([len(s) for s in streams], dtype=np.int32)), raw, st, 1 << 20)
    t.cuda.synchronize(dc.dev)
    assert st.tolist() == [0] * 16 + [M.E_EMPTY, M.E_TRUNCATED, 0]
    assert raw.tolist() == [len(f[3]) for f in fx] + [0, 0, 0]


# ---- edge.bin ------------------------------------------------------------------------------------------------------
def test_every_edge_input_in_one_batch(dc):
    inputs, _ = M.edge()
    streams = [i[4] for i in inputs]
    outs, st, lens, nrec, route = check(dc, streams)
    assert st == [0] * len(streams)
    for (name, data, want_lens, flags, stream, size, digest), out, got in zip(inputs, outs, lens):
        assert len(out) == size and got == want_lens, name
        assert out == data if data is not None else hashlib.sha256(out).digest() == digest, name
    # both table homes, the reversal, several parameter blocks, duplicates
    assert route["tab_global"] == 2 and route["tab_lds"] == len(streams) - 3 and route["do_rev"] == 2      # ("empty" decodes nothing)
    assert route["multi_param"] >= 8 and route["dup"] >= 3


def test_every_damaged_stream_and_the_undefined_cases(dc):
    _, damaged = M.edge()
    streams = [s for s, _ in damaged] + M.model_undefined() + [s for s, _ in M.model_refused()]
    outs, st, lens, nrec, route = check(dc, streams)
    for i, (stream, ans) in enumerate(damaged):
        if ans is None:
            assert st[i] != 0, i
        else:
            assert st[i] == 0 and (len(outs[i]), nrec[i], hashlib.sha256(outs[i]).hexdigest()) == ans, i
    at = len(damaged)
    assert st[at:at + len(M.model_undefined())] == [M.E_TABLE] * len(M.model_undefined())       # refused, not decoded
    assert all(s != 0 for s in st[at:])


# ---- confinement: refused streams, lengths slots of 0, 1 and exact -------------------------------------------------
def test_nothing_is_written_outside_the_slots(dc):
    inputs, damaged = M.edge()
    streams = [i[4] for i in inputs if i[5] <= 4400] + [s for s, a in damaged[:60]] + M.model_undefined()
    res, _ = expect(streams, [1 << 22] * len(streams))
    for mode in (0, 1, "exact", "roomy"):
        len_caps = [0 if mode == 0 else 1 if mode == 1 else len(r[2]) + (5 if mode == "roomy" else 0) for r in res]
        check(dc, streams, len_caps=len_caps)                        # capacities: exactly the stored sizes
    check(dc, streams, len_caps=None)


# ---- second trips ----------------------------------------------------------------------------------------------------
def test_two_slots_five_streams_of_different_max_sym(dc):
    inputs, _ = M.edge()
    by_name = {i[0]: i[4] for i in inputs}
    streams = [by_name[k] for k in ("width256", "width2", "nparam9", "width65", "rev")]
    assert len({M.parse(s)[1].max_sym for s in streams}) == 5
    dc.set_fqz_limits(max_slots=2)
    try:
        check(dc, streams)                                           # wave 0 decodes streams 0, 2, 4; wave 1 streams 1, 3
        check(dc, streams[::-1])
    finally:
        dc.set_fqz_limits()


def test_a_slot_limit_below_a_streams_max_sym_refuses_that_stream(dc):
    inputs, _ = M.edge()
    by_name = {i[0]: i[4] for i in inputs}
    streams = [by_name["width64"], by_name["width65"]]
    dc.set_fqz_limits(max_sym=63)
    try:
        outs, st, lens, nrec, route = run_dev(dc, streams, [3000, 3000])
    finally:
        dc.set_fqz_limits()
    assert st == [0, M.E_UNSUPPORTED] and outs[0] == answer(streams[0])[1] and route["streams"] == 1


def test_eight_streams_walk_in_chunks_under_a_low_workspace_ceiling(dc, fx):
    streams = [fx[k][2] for k in (12, 13, 14, 15)] + [i[4] for i in M.edge()[0][:4]]
    was = dc.get_option("max_workspace_mb")
    dc.set_fqz_limits(max_sym=50)                                    # a slot: 65,536 x (4 x 52 + 4) bytes = 13.25 MiB
    dc.set_option("max_workspace_mb", 48)                            # three slots and the stage arena: chunks of 3, 3, 2
    try:
        outs, st, lens, nrec, route = check(dc, streams, want_chunks=3)
    finally:
        dc.set_option("max_workspace_mb", was)
        dc.set_fqz_limits()
    assert st == [0] * 8 and outs[:4] == [fx[k][3] for k in (12, 13, 14, 15)]


# ---- capacity and total_out_size -------------------------------------------------------------------------------------
def test_one_byte_short_is_a_capacity_error_and_leaves_the_slot_untouched(dc):
    import numpy as np
    from test_gpu_confinement import Layout
    inputs, _ = M.edge()
    streams = [i[4] for i in inputs if 0 < i[5] <= 4400][:12]
    sizes = [len(answer(s)[1]) for s in streams]
    caps = [n - 1 if k % 2 else n for k, n in enumerate(sizes)]
    outs, st, lens, nrec, route = check(dc, streams, caps)
    assert st == [M.E_CAPACITY if k % 2 else 0 for k in range(len(streams))]
    # the refused slots still hold the pattern: run once more and look inside them
    import torch as t
    lay = Layout(caps)
    d_out = t.from_numpy(lay.pattern.copy()).to(dc.dev)
    arena_in = np.frombuffer(b"".join(streams) + bytes(16), dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(s) for s in streams[:-1]]).astype(np.int64)
    up = lambda a: t.from_numpy(a).to(dc.dev)
    osz, stt = (t.full((len(streams),), -7, dtype=t.int32, device=dc.dev) for _ in range(2))
    dc.fqz_uncompress(up(arena_in), up(off), up(np.array([len(s) for s in streams], dtype=np.int32)), d_out, up(lay.offs.copy()),
                      up(np.array(caps, dtype=np.int32)), osz, stt, max(len(s) for s in streams), max(caps))
    t.cuda.synchronize(dc.dev)
    got = d_out.cpu().numpy()
    for k, (o, c) in enumerate(zip(lay.offs, caps)):
        if k % 2:
            assert (got[o:o + c] == lay.pattern[o:o + c]).all(), k


def test_total_out_size_exact_decodes_all_and_one_less_refuses_the_last(dc):
    inputs, _ = M.edge()
    streams = [i[4] for i in inputs if 0 < i[5] <= 4400][:10]
    sizes = [len(answer(s)[1]) for s in streams]
    outs, st, _, _, _ = run_dev(dc, streams, sizes, total=sum(sizes))
    assert st == [0] * 10 and outs == [answer(s)[1] for s in streams]
    outs, st, _, _, route = run_dev(dc, streams, sizes, total=sum(sizes) - 1)
    assert st == [0] * 9 + [M.E_UNSUPPORTED] and outs[:9] == [answer(s)[1] for s in streams[:9]] and route["streams"] == 9
