"""Damaged arith_dynamic streams through the device call and the host batch (include/rans4x16_hip.h part 2g): the
reference-answered ones of tests/golden/arith/edge.bin, a few hundred made from model-coded streams of at most 8 KB, and
some sixty of streams whose rows live in global memory and whose payload is longer than the coder's input window.
Every case is compared and none is left out: a refused one must be refused with the walk's status, an accepted one must
match the expected bytes, the neighbours' slots and the guard bytes must be untouched (arith_gpu.run_dev).  The inputs
are bytes the decoder must survive; each is run once."""
import hashlib

import pytest

import arith_cases as K
import arith_model as M
from arith_gpu import check

pytestmark = pytest.mark.gpu
PLANES, STRIPE_OUT = 8, 8192


@pytest.fixture(scope="module")
def dc():
    import htscodecs_amd as H
    return H.DeviceCodec(0)


def _sized(cases):
    """the device call has no 'out == NULL': such a case gets the capacity the reference allocates for it, the size the
    stream stores (arith_dynamic.c:893, :984; the vectors hold no such case for a stream that stores none)"""
    out = []
    for s, cap in cases:
        if cap is None:
            cap = K.claim(s)[1]
            assert cap is not None and cap <= 1 << 20
        out.append((s, cap))
    return out


def test_edge_bin_damaged_streams_through_the_device_call(dc):
    _, damaged = K.edge()
    cases = _sized([(s, c) for s, c, _ in damaged])
    outs, st, _ = check(dc, [s for s, _ in cases], [c for _, c in cases], planes=PLANES, stripe_out=STRIPE_OUT)
    # the reference's own answers, every case (the model's were asserted by check)
    for i, ((s, _, answer), out, status) in enumerate(zip(damaged, outs, st)):
        if answer is None:
            assert status != 0, i
        else:                                                        # (none of them lies beyond the reservation)
            assert status == 0 and (len(out), hashlib.sha256(out).hexdigest()) == answer, i


def test_model_made_damaged_streams_through_the_device_call(dc):
    cases = _sized(K.model_damaged())
    assert len(cases) >= 290
    _, st, _ = check(dc, [s for s, _ in cases], [c for _, c in cases], planes=PLANES, stripe_out=STRIPE_OUT)
    assert 40 < sum(1 for x in st if x) < len(st) - 40                # both verdicts are well represented


def test_damaged_streams_of_the_global_home_through_the_device_call(dc):
    """bases with an alphabet above 84 and more than 1 KiB of payload: the guards of the step with the rows in global
    memory and the input window past its first refill (test_arith_inputs_cpu.py holds the list to that)"""
    cases = K.global_damaged()
    assert len(cases) >= 60
    _, st, route = check(dc, [s for s, _ in cases], [c for _, c in cases], planes=PLANES, stripe_out=STRIPE_OUT)
    assert route["o1_global"] >= 30 and any(st) and not all(st)


def test_damaged_streams_through_the_host_batch_and_the_single_call(dc):
    from htscodecs_amd import codec
    _, damaged = K.edge()
    cases = [(s, c) for s, c, _ in damaged if c is not None] + _sized(K.model_damaged())
    outs, st = codec.arith_uncompress_batch([s for s, _ in cases], [c for _, c in cases])
    for i, ((s, cap), out, status) in enumerate(zip(cases, outs, st)):
        wst, want = M.uncompress_to(s, cap)
        assert status == wst, (i, status, wst, s[:12].hex(), cap)
        assert out == (want if wst == 0 else None), i
    # out == NULL: the size comes from the stream
    for i, (s, cap, answer) in enumerate(damaged):
        if cap is None:
            out = codec.arith_uncompress(s)
            if answer is None:
                assert out is None, i
            else:
                assert out is not None and (len(out), hashlib.sha256(out).hexdigest()) == answer, i
