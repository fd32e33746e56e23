"""fqzcomp_qual encoding on the device (htscodecs_amd/csrc/r4x16_fqz_enc.hip, include/rans4x16_hip.h part 2j).

The expected bytes are the reference's own: the 16 streams of tests/golden/fqzcomp (parameters picked by the library's
host pick, which test_fqz_enc_cpu.py holds to the same streams) and every input of edge.bin and records.bin whose bytes
are kept (parameter bytes cut from the reference's stream, lengths and flags from the file), and the inputs those files
keep as a digest only, recovered from the reference's stream by the model's decoder and held to the digest
(fqz_enc_model.hashed_vectors).  Where no reference stream
exists - the slice-scale input of census_slice(), the vers 3 drop-in case, refusals - the answer is the Python model's
(fqz_enc_model.py), which test_fqz_enc_cpu.py holds to all of the above.  Everything is exact.  Every device call runs in
the confinement layout of fqz_enc_gpu.run_dev, with set_fqz_limits lowered to the batch's max_sym."""
import numpy as np
import pytest

import arith_model as A
import fqz_enc_model as E
import fqz_model as M
from fqz_enc_gpu import check, decode_back, run_dev, answer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dc():
    import htscodecs_amd as H
    return H.DeviceCodec(0)


@pytest.fixture(scope="module")
def picked():
    """the 16 fixtures as blocks under picked parameters: [(file name, block, the reference's stream)]"""
    from htscodecs_amd import codec
    res = []
    for fn, strat, stream, data, lens, flags in E.fixture_slices():
        st, par, l2, f2 = codec.fqz_pick_parameters(data, lens, flags, 4, strat)
        assert st == 0
        res.append((fn, (data, l2, f2, par), stream))
    return res


@pytest.fixture(scope="module")
def kept():
    return [(name, (data, lens, flags, E.params_of(stream)), stream) for name, data, lens, flags, stream in E.kept_vectors()]


# ---- 1. the reference's 16 streams ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(16))
def test_each_fixture_alone_is_the_references_stream(dc, picked, k):
    fn, block, stream = picked[k]
    outs, st, route = check(dc, [block])
    assert st == [0] and outs[0] == stream, fn
    assert route["streams"] == route["tab_lds"] == 1 and route["tab_global"] == route["do_rev"] == route["multi_param"] == 0
    assert route["dup"] == 0                                         # (qvar asks for duplicates and has none)


def test_the_16_fixtures_as_one_batch_and_back(dc, picked):
    outs, st, route = check(dc, [b for _, b, _ in picked])
    assert st == [0] * 16 and outs == [s for _, _, s in picked]
    assert route["streams"] == route["tab_lds"] == 16 and route["dup"] == 0
    decode_back(dc, outs, [b for _, b, _ in picked])


def test_the_16_fixtures_through_the_host_batch_with_params_null(picked):
    import htscodecs_amd as H
    sl = E.fixture_slices()
    outs, st, lens, flags = H.fqz_compress_batch([s[3] for s in sl], [s[4] for s in sl], [s[5] for s in sl], 4, 0, params=None)
    # one strat a call: the batch takes strat 0 for all; the four .0 files are the reference's answers
    for (fn, strat, stream, data, l0, f0), out, s, fl in zip(sl, outs, st, flags):
        assert s == 0 and fl == [f & 0xffff for f in f0]
        if strat == 0:
            assert out == stream, fn
    for want_strat in (1, 2, 3):
        some = [s for s in sl if s[1] == want_strat]
        outs, st, _, _ = H.fqz_compress_batch([s[3] for s in some], [s[4] for s in some], [s[5] for s in some], 4, want_strat)
        assert st == [0] * len(some) and outs == [s[2] for s in some]


def test_the_single_call_on_two_fixtures():
    import htscodecs_amd as H
    for fn, strat, stream, data, lens, flags in E.fixture_slices():
        if fn in ("q40+dir.1", "qvar.0"):
            got = H.fqz_compress(data, lens, flags, 4, strat)
            assert got is not None and got[0] == stream and got[1] == lens and got[2] == flags, fn
    assert H.fqz_compress(b"\x05" * 10, [10], [0], 4, 0, gp=1) is None       # a parameter struct is not taken


# ---- 2. edge.bin and records.bin -------------------------------------------------------------------------------------
def test_every_kept_input_of_edge_and_records_in_one_batch_and_back(dc, kept):
    outs, st, route = check(dc, [b for _, b, _ in kept])
    assert st == [0] * len(kept)
    for (name, b, stream), out in zip(kept, outs):
        assert out == stream, name
    assert route == {"streams": 26, "tab_lds": 24, "tab_global": 2, "do_rev": 4, "multi_param": 10, "dup": 4}
    decode_back(dc, outs, [b for _, b, _ in kept])


def test_every_hashed_input_of_edge_and_records_in_one_batch_and_back(dc):
    """the tie after a halving in a quality row (halve_tie, halve_tie2), a record of 70,000 bytes (lens: the third `len`
    byte, a window refill and the front's sum beyond 65,535) and the slices of thousands of records (records, bit_swap,
    rev_trips: the per-record models past their halvings) - against the reference's own streams"""
    hashed = E.hashed_vectors()
    assert {h[0] for h in hashed} >= {"edge:halve_tie", "edge:halve_tie2", "edge:halve", "edge:lens", "records:records", "records:rev_trips",
                                      "records:bit_swap"}
    assert max(max(h[2]) for h in hashed) == 70000 and max(len(h[2]) for h in hashed) == 6700
    blocks = [(data, lens, flags, E.params_of(stream)) for name, data, lens, flags, stream in hashed]
    outs, st, route = check(dc, blocks)
    assert st == [0] * len(hashed)
    for (name, data, lens, flags, stream), out in zip(hashed, outs):
        assert out == stream, name
    assert route["streams"] == route["tab_lds"] == len(hashed) and route["do_rev"] == 3 and route["multi_param"] == 1 and route["dup"] >= 2
    decode_back(dc, outs, blocks)


# ---- 3. slot reuse ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_slots", [1, 2])
def test_a_wave_takes_its_second_and_third_stream(dc, kept, picked, max_slots):
    blocks = [b for _, b, _ in kept] + [picked[15][1]]
    want = [s for _, _, s in kept] + [picked[15][2]]
    outs, st, route = check(dc, blocks, max_slots=max_slots)
    assert st == [0] * len(blocks) and outs == want


# ---- the per-record models past their halvings (no reference stream: the model) -----------------------------------------
def test_census_slice_is_the_models_stream_and_decodes_back(dc):
    block = E.census_slice()
    outs, st, route = check(dc, [block])
    assert st == [0] and route["do_rev"] == route["multi_param"] == route["dup"] == 1
    decode_back(dc, outs, [block])


# ---- 5. capacity -----------------------------------------------------------------------------------------------------
def test_capacity_size_minus_one_size_and_cap(dc, kept, picked):
    good = {name: b for name, b, _ in kept}
    # (dup_chain and dup_long take duplicates: a stream refused for its last bytes counts none)
    blocks = [b for _, b, _ in kept if len(b[0])][:6] + [good["edge:dup_chain"], good["records:dup_long"], picked[12][1]]
    sizes = [len(answer(b)[1]) for b in blocks]
    many = [b for b in blocks for _ in range(3)]
    caps = [c for b, n in zip(blocks, sizes) for c in (n - 1, n, E.cap(len(b[0]), len(b[1]), len(b[3])))]
    outs, st, route = check(dc, many, caps)
    assert st == [M.E_CAPACITY, 0, 0] * len(blocks)


def test_the_cap_is_the_librarys():
    from htscodecs_amd import codec
    for args in ((0, 0, 9), (1, 1, 9), (151000, 1000, 300), (1 << 31, 1 << 20, 4096)):
        assert codec.fqz_compress_cap(*args) == E.cap(*args)


# ---- 7. refusals, each beside good blocks ----------------------------------------------------------------------------
def hostile_blocks(kept, picked):
    good = {name: b for name, b, _ in kept}
    res = []
    data, lens, flags, par = good["edge:nparam3+stab"]
    res.append(("sum", (data, lens[:-1] + [lens[-1] + 1], flags, par), M.E_SIZE))
    res.append(("sum_short", (data, lens[:-1], flags[:-1], par), M.E_SIZE))
    res.append(("len0", (data, [0] + lens, [flags[0]] + flags, par), M.E_SIZE))
    res.append(("no_records", (data, [], [], par), M.E_SIZE))
    res.append(("sel_above_max_sel", (data, lens, [flags[0] | (200 << 16)] + flags[1:], par), M.E_CONTEXT))
    one = M.store_parameters(M.gparams([M.param(max_sym=12, qbits=4, qshift=2, do_sel=True)], gflags=M.GFLAG_HAVE_STAB, max_sel=2,
                                       stab=[0, 0] + [1] * 254))
    small = bytes([1, 2, 3, 4] * 10)
    res.append(("stab_beyond_nparam", (small, [20, 20], [0, 2 << 16], one), M.E_CONTEXT))
    res.append(("stab_inside_nparam", (small, [20, 20], [0, 1 << 16], one), 0))
    qm = M.store_parameters(M.gparams([M.param(qbits=4, qshift=2, qmap_of=[1, 2, 3, 4])]))
    res.append(("qmap_has_it", (small, [40], [0], qm), 0))
    res.append(("outside_qmap", (small[:-1] + b"\x07", [40], [0], qm), M.E_CONTEXT))
    ms = M.store_parameters(M.gparams([M.param(max_sym=8, qbits=4, qshift=2)]))
    res.append(("at_max_sym", (small[:-1] + b"\x08", [40], [0], ms), 0))
    res.append(("above_max_sym", (small[:-1] + b"\x09", [40], [0], ms), M.E_CONTEXT))
    for k, (s, site) in enumerate(M.model_refused()):
        q = A.var_get(s, 0, len(s))[0] if s else 0
        res.append(("walk:%s:%d" % (site, k), (small, [40], [0], s[q:]), None))
    for k, s in enumerate(M.model_undefined()):
        q = A.var_get(s, 0, len(s))[0]
        res.append(("undefined:%d" % k, (small, [40], [0], s[q:]), M.E_TABLE))
    multi = M.store_parameters(M.gparams([M.param(max_sym=8, qbits=4, qshift=2)] * 2, gflags=M.GFLAG_HAVE_STAB, max_sel=0, stab=[0] * 256))
    res.append(("multi_param_without_sel_model", (small, [40], [0], multi), M.E_TABLE))
    res.append(("bytes_left_over", (small, [40], [0], ms + b"\x00"), M.E_UNSUPPORTED))
    return res


def test_refusals_beside_good_blocks(dc, kept, picked):
    bad = hostile_blocks(kept, picked)
    good = [b for _, b, _ in kept][:8]
    blocks, want = [], []
    for k, (name, b, st) in enumerate(bad):
        blocks += [b, good[k % len(good)]]
        want += [st, 0]
    outs, st, route = check(dc, blocks)
    for k, (name, b, w) in enumerate(bad):
        assert st[2 * k] == w if w is not None else st[2 * k] != 0, (name, st[2 * k])
        assert st[2 * k + 1] == 0, name


def test_max_sym_above_the_limit_and_a_block_above_max_in_size(dc, kept, picked):
    good = {name: b for name, b, _ in kept}
    blocks = [good["edge:width5"], good["edge:width64"], good["edge:width4"]]
    outs, st, route = check(dc, blocks, max_sym_limit=4)
    assert st == [0, M.E_UNSUPPORTED, 0]
    # width64 is 3,000 bytes, the others 600: announced 1,000
    want = [answer(b)[1] for b in blocks]
    caps = [len(w) for w in want]
    dc.set_fqz_limits(0, 63)
    try:
        outs, st, route = run_dev(dc, blocks, caps, max_in=1000)
    finally:
        dc.set_fqz_limits(0, 0)
    assert st == [0, M.E_UNSUPPORTED, 0] and outs[0] == want[0] and outs[2] == want[2] and route["streams"] == 2
    for kw in (dict(max_par=8), dict(max_rec=2)):
        dc.set_fqz_limits(0, 63)
        try:
            outs, st, route = run_dev(dc, blocks, caps, **kw)
        finally:
            dc.set_fqz_limits(0, 0)
        assert st == [M.E_UNSUPPORTED] * 3 and route["streams"] == 0


# ---- 8. vers 3 through the drop-in path ------------------------------------------------------------------------------
def test_vers_3_drop_in_with_mixed_reverse_flags(dc):
    import htscodecs_amd as H
    from htscodecs_amd import codec
    data, lens, flags = E.drop_in_case()
    got = H.fqz_compress(data, lens, flags, 3, 0)                    # (the wrapper asserts that the input is unchanged)
    assert got is not None
    stream, l2, f2 = got
    assert l2 == lens and f2 == flags
    st, par, l3, f3 = codec.fqz_pick_parameters(data, lens, flags, 3, 0)
    st_h, h = E.parse_params(par)
    assert st == 0 and st_h == 0 and h.gflags & M.GFLAG_DO_REV
    assert stream == E.compress(data, l3, f3, par)
    back = H.fqz_decompress(stream, nlengths=len(lens))
    assert back == (data, lens)
    decode_back(dc, [stream], [(data, lens, flags, par)])
