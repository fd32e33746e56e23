"""rans4x16_hip_residency over its whole input grid against a table recorded on an MI355X at the commit named in the
fixture (tests/golden/residency_table.json): every alphabet size, both orders, both table shifts, decode with and without
option dec_short_ring, encode, and the R4X16_RES_SHORT / R4X16_RES_MID kinds - the refusals and the reported CU count
included.  The answers are host arithmetic on the launchers' class tables and the one residency rule
(sched_resident_per_cu); a change to either that moves a stream kind to another class or count shows here."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

RES_SHORT, RES_MID = 2, 4            # include/rans4x16_hip.h R4X16_RES_*
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "residency_table.json")


def _expected_cases():
    """(decode, kind, order, shift, dec_short_ring): what the table has to cover."""
    want = set()
    for order in (0, 1):
        for shift in (10, 12):
            want |= {(1, 0, order, shift, 0), (1, 0, order, shift, 1), (0, 0, order, shift, 0),
                     (1, RES_SHORT, order, shift, 0), (0, RES_SHORT, order, shift, 0), (1, RES_MID, order, shift, 0)}
    return want


def test_residency_answers_match_the_recorded_table():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd as H
    H.load()
    with open(GOLDEN) as f:
        tab = json.load(f)
    assert tab["columns"] == ["decode", "kind", "order", "shift", "dec_short_ring"]
    assert tab["nsym"] == [1, 256]
    assert {tuple(c) for c in tab["cases"]} == _expected_cases() and len(tab["cases"]) == len(_expected_cases())
    dc = H.DeviceCodec(0)
    refusals = 0
    for case, streams, lanes in zip(tab["cases"], tab["streams_per_cu"], tab["lanes_per_wave"]):
        decode, kind, order, shift, short_ring = case
        assert len(streams) == 256 and len(lanes) == 256
        dc.set_option("dec_short_ring", short_ring)
        for nsym in range(1, 257):
            try:
                got = dc.residency(bool(decode), nsym, order, shift=shift, kind=kind)
            except RuntimeError:
                got = (-1, -1, tab["compute_units"])          # a refusal
                refusals += 1
            assert got == (streams[nsym - 1], lanes[nsym - 1], tab["compute_units"]), (case, nsym)
    assert refusals == sum(s.count(-1) for s in tab["streams_per_cu"])
