"""The quad's emit count of the encode chain's packed-row step on the device (htscodecs_amd/csrc/r4x16_enc_chain.h:
ENC_TRIP_STEP's half-wave masks and DPP move, EncOutT::trip_enter / trip_leave, flush_pipelined<true>) against the CPU
oracle, byte for byte: rans4x16_hip_compress_dev with order 1 and the symbol records off, output slots laid out between
guard bytes (tests/test_gpu_confinement.py's arenas: nothing outside a slot may change, and the input may not either).

What the count depends on: the half of the wave a quad lies in (lanes 0..31 / 32..63), what the other quads of the wave
emit, the words written so far (the ring's wrap at 64, the flush at every 32) and the edges of the pipelined loop, where
`written` becomes wm1 and back (phase A in front of it codes n & 3 bytes, the single steps behind it the rest).
A wave holds the streams of a workgroup in slot order, four lanes each; the launcher gives a small batch workgroups of one
wave with eight streams, so quads reach lanes 32..63 only in large batches or under the tuning options enc_qpw /
enc_waves, which act on the class of the 46-symbol tables once the batch is large enough for workgroups of that size
(`shape` below restates enc_rows_shape's rule).  The 20-symbol alphabet's class therefore runs with 1 and 8 streams in a
wave here, the 46-symbol one with 1, 8, 9 and 12.
Every case asserts its route: packed rows of the short-index kind ("packed_freq"; 0 for the block that reaches byte 128)
and the streams counted by waves of the affine body ("packed_affine")."""
import numpy as np
import pytest

from test_enc_affine_cpu import affine_of, alpha_of
from test_gpu_confinement import _Guarded, _expect
from test_gpu_enc_affine import block, run_of
from test_gpu_enc_step import _want, takes_packed

LENGTHS = (4092, 4096, 4100, 4099, 65537)


def is_affine(raw):
    return affine_of(alpha_of(raw), 0 in raw) != 0


def shape(nblk, cus, force_qpw, force_waves, class_qpw=45):
    """(streams per workgroup, waves, streams per wave) of the tuned packed class: enc_rows_shape's rule restated."""
    qpw = force_qpw or class_qpw
    want = max(8, (((3 * nblk + 2) // 3 + cus - 1) // cus + 3) & ~3)
    qpw = min(qpw, want)
    waves = force_waves or min(4, (qpw + 7) // 8)
    return qpw, waves, (qpw + waves - 1) // waves


@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd


def check(H, opts, raws, affine, short=None, enc_affine=1, enc_qpw=0, enc_waves=0):
    """One call over `raws`: the oracle's bytes in every slot, nothing written outside the slots, the input unchanged,
    and the route; `affine`: the streams counted by waves of the affine body, `short`: those of the short-index kind
    (default: all)."""
    opts.set("enc_direct", 0)
    opts.set("enc_affine", enc_affine)
    opts.set("enc_qpw", enc_qpw)
    opts.set("enc_waves", enc_waves)
    dc = H.DeviceCodec(0)
    dc.set_option("route_count", 1)
    assert dc.get_option("enc_qpw") == enc_qpw and dc.get_option("enc_waves") == enc_waves
    assert all(takes_packed(r) for r in set(raws))
    caps = [H.rans_compress_bound_4x16(len(r), 1) for r in raws]
    G = _Guarded(dc.dev, raws, caps, [("size", len(r)) for r in raws])
    dc.route_read("encode"), dc.route_read("encode_body")
    rc = dc.L.rans4x16_hip_compress_dev(dc.ctx.h, G.n, *G.ptrs(), 1, None, G.max_in, dc._stream())
    assert rc == 0, dc.ctx.error()
    label = ("encode", len(raws), enc_qpw, enc_waves)
    st, osz, got = G.results(label)
    _expect(label, G, st, osz, got, [_want(r) for r in raws])
    route, body = dc.route_read("encode"), dc.route_read("encode_body")
    assert route["records"] == 0 and route["packed"] == len(raws), route
    assert route["packed_freq"] == (len(raws) if short is None else short), route
    assert body["packed_affine"] == affine, (body, affine)


@pytest.mark.gpu
@pytest.mark.parametrize("enc_affine", [1, 0], ids=["affine", "look-up"])
@pytest.mark.parametrize("ns", [46, 20])
def test_one_and_eight_streams_in_a_wave(H, opts, ns, enc_affine):
    """Every length alone (one quad at lanes 0..3, the other sixty lanes code neutral symbols), then eight blocks of one
    length (quads at lanes 0..31)."""
    a = run_of(ns, 33)
    for n in LENGTHS:
        check(H, opts, [block(n, a)], enc_affine, enc_affine=enc_affine)
    for n in LENGTHS[:4]:
        check(H, opts, [block(n, a, seed=i) for i in range(8)], 8 * enc_affine, enc_affine=enc_affine)


@pytest.mark.gpu
@pytest.mark.parametrize("enc_affine", [1, 0], ids=["affine", "look-up"])
@pytest.mark.parametrize("spw", [9, 12])
def test_quads_in_the_upper_half_of_the_wave(H, opts, spw, enc_affine):
    """Nine and twelve streams in a wave: quads at lanes 32..35 and up to 44..47.  One wave per workgroup of `spw` streams
    needs a batch of more than eight blocks per compute unit; the blocks are twenty-four distinct ones of the four short
    lengths, repeated, so the waves at the borders between two lengths hold streams that end at different trips."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nblk = 8 * cus + 24
    assert shape(nblk, cus, spw, 1) == (spw, 1, spw) and shape(8, cus, spw, 1)[2] == 8
    a = run_of(46, 33)
    pool = [block(n, a, seed=20 + i) for i in range(6) for n in LENGTHS[:4]]
    raws = [pool[i % len(pool)] for i in range(nblk)]
    check(H, opts, raws, nblk * enc_affine, enc_affine=enc_affine, enc_qpw=spw, enc_waves=1)


@pytest.mark.gpu
@pytest.mark.parametrize("enc_affine", [1, 0], ids=["affine", "look-up"])
@pytest.mark.parametrize("ns", [46, 20])
def test_unequal_lengths_in_one_wave(H, opts, ns, enc_affine):
    """Eight streams of 140 to 65,537 bytes in one wave: a lane past its end codes neutral symbols beside live ones for
    most of the longest stream's trips, and every stream enters and leaves the pipelined loop with its own count."""
    a = run_of(ns, 33)
    lens = (4096, 140, 65537, 4099, 1023, 12345, 4092, 33001)
    check(H, opts, [block(n, a, seed=40 + i) for i, n in enumerate(lens)], len(lens) * enc_affine, enc_affine=enc_affine)


@pytest.mark.gpu
def test_gapped_alphabet_takes_the_look_up_body(H, opts):
    """A byte missing from the middle of the run: no affine alphabet, the look-up body of the same kernel - alone, eight
    to a wave, and beside an affine block (the wave then takes the look-up body for both)."""
    gap = np.delete(run_of(47, 33), 20)
    raws = [block(n, gap, seed=50 + i) for i, n in enumerate(LENGTHS)]
    assert not any(is_affine(r) for r in raws)
    for r in raws:
        check(H, opts, [r], 0)
    check(H, opts, raws[:4] + [block(4096, gap, seed=60 + i) for i in range(4)], 0)
    check(H, opts, [raws[1], block(4096, run_of(46, 33), seed=61)], 0)


@pytest.mark.gpu
def test_block_that_reaches_byte_128_takes_the_full_index(H, opts):
    """A run across byte 128: packed rows of the full-index kind (k_enc_chain<true, true, false>, which keeps emit16q)."""
    high = run_of(46, 129 - 23)
    raws = [block(n, high, seed=70 + i) for i, n in enumerate(LENGTHS)]
    assert all(max(r) >= 128 for r in raws)
    check(H, opts, raws, 0, short=0)


def test_cases_are_what_they_claim():
    """No GPU: alphabets, table precision, affinity, the loop's stages, and the shape rule for 256 and 304 compute units."""
    for ns in (46, 20):
        for n in LENGTHS:
            raw = block(n, run_of(ns, 33))
            assert len(alpha_of(raw)) == ns and max(raw) < 128 and is_affine(raw) and takes_packed(raw), (ns, n)
    assert {n & 3 for n in LENGTHS} == {0, 1, 3} and {(((n >> 2) - 1) >> 3) & 3 for n in LENGTHS} >= {0, 3}
    # more than 32 words per chain: every stream wraps the ring and flushes (uniform draws over 20 symbols: > 4 bits a byte)
    assert all(len(_want(block(n, run_of(20, 33)))) > 4 * 2 * 64 for n in LENGTHS)
    for cus in (256, 304):
        for spw in (9, 12):
            assert shape(8 * cus + 24, cus, spw, 1) == (spw, 1, spw)
        assert shape(8, cus, 12, 1) == (8, 1, 8) and shape(8, cus, 0, 0) == (8, 1, 8) and shape(45 * cus, cus, 0, 0) == (45, 4, 12)
