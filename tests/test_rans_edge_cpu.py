"""rANS 4x16 and 4x8 against reference-made edge and damaged vectors, the half that needs no GPU: tests/golden/rans/edge.bin
is what its README says; the oracle (oracle/rans4x16_oracle.c, rans4x8_oracle.c) writes every stream the REFERENCE wrote
for the fixture's inputs, byte for byte, and decodes every one of them; for every damaged stream whose answer from the
reference is stable it gives that answer, or the stream's bytes satisfy one of rans_edge_cases.DEVIATIONS; every entry of
that list has a member in the fixture; and, where oracle/_ref/rans_ref exists (build() makes it where a reference tree
is), 1,000 random inputs and 2,000 damaged streams go through the reference and the oracle live, by the same rule.

The fixture is read once per session and not changed."""
import collections
import os
import random
import re

import pytest

import rans_edge_cases as X
from test_oracle4x8 import Codec8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRANCHES = ("size_", "stripe_", "pack_", "rle_", "rle99_", "rlemeta_", "cat_explicit", "catfall_", "o1_alphabet_run_", "o1table_", "o1shift_",
            "norm_", "large_", "x8_size_", "x8_alphabet_", "x8_symbol_run_", "x8_freq_", "x8_large")


@pytest.fixture(scope="module")
def orc8(oracle):
    return Codec8(oracle.lib, "orc8_")


def oracle_answer(oracle, orc8, op, capacity, stream):
    """REFUSED or the bytes: the oracle called as the reference was (rans_edge_cases: OP_U16_TO, OP_U16, OP_U8)."""
    if op == X.OP_U8:
        got = orc8.uncompress(stream)
    elif op == X.OP_U16_TO:
        got = oracle.uncompress(stream, capacity=capacity)
    else:
        got = oracle.uncompress_malloc(stream)
    return X.REFUSED if got is None else got


def excused(codec, stream, capacity, reference, mine):
    """The DEVIATIONS entries that cover the oracle's answer `mine` where it is not the reference's stable answer
    `reference` (bytes, or a digest): the reference accepts; the oracle refuses and an entry on which it "refuses" holds, or
    it accepts with other bytes and an entry on which it gives "other" bytes holds.  An entry that is the device's alone
    ("follows") covers nothing here, and nothing covers an answer to a stream the reference refuses."""
    if reference == X.REFUSED:
        return []
    kind = "refuses" if mine == X.REFUSED else "other"
    return [x for x in X.deviation(codec, stream, capacity) if x.oracle == kind]


def same_answer(reference, mine):
    if reference == X.REFUSED or mine == X.REFUSED:
        return mine == reference
    return mine == reference if isinstance(reference, bytes) else X.digest(mine) == reference


def judge(codec, stream, capacity, reference, mine):
    """None where `mine` is the reference's answer or a deviation covers it, else a description."""
    if same_answer(reference, mine) or excused(codec, stream, capacity, reference, mine):
        return None
    say = lambda a: "refused" if a == X.REFUSED else "%d bytes" % len(a) if isinstance(a, bytes) else "%d bytes (digest)" % a[0]
    return "4x%d, capacity %d, %s: reference %s, oracle %s" % (codec, capacity, stream[:24].hex(), say(reference), say(mine))


def test_edge_bin_is_what_its_readme_says():
    fx = X.load()
    assert os.path.getsize(X.EDGE) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "fqzcomp", "edge.bin")) == 208487
    with open(X.README) as f:
        text = f.read()
    rows = re.findall(r"^\| `([a-z0-9_]+)` \| ([^|]+) \| ([^|]+) \| (\d+) \| ([0-9a-fx:, ]+) \|$", text, flags=re.M)
    assert [r[0] for r in rows] == [c.name for c in fx.cases] and len({c.name for c in fx.cases}) == len(fx.cases) >= 150
    for c, (_, branch, side, size, lens) in zip(fx.cases, rows):
        assert branch.strip() and side.strip(), c.name
        n = c.data[0] if c.spec else len(c.data)
        assert int(size) == n and (n <= 4099) == all(isinstance(v.stream, bytes) for v in c.vectors), c.name
        assert n <= 70000 and c.codec in (16, 8), c.name
        assert lens.strip() == ", ".join("%#x: %d" % (v.order, len(v.stream) if isinstance(v.stream, bytes) else v.stream[0]) for v in c.vectors), c.name
        assert any(c.name.startswith(b) for b in BRANCHES), c.name
    assert all(any(c.name.startswith(b) for c in fx.cases) for b in BRANCHES)
    # both sides of every family's decision are there
    for prefix in ("rle99_", "rlemeta_", "catfall_", "o1table_", "o1shift_"):
        sides = [r[2] for r in rows if r[0].startswith(prefix)]
        assert any("the last of the family" in s for s in sides) and any("the first with" in s for s in sides), prefix
    # the damaged streams: 600 a codec from reference-made streams of 30 to 1,500 bytes, most of them stable
    for codec in (16, 8):
        ds = X.damaged_streams(codec)
        assert len(ds) == 600
        stable = [d for d, _ in ds if d.answer is not None]
        assert len(stable) >= 400 and sum(d.answer != X.REFUSED for d in stable) >= 100
        assert all(30 <= len(s) <= 1500 for c, s in fx.bases if c == codec)
        if codec == 8:
            assert all(len(s) < 9 or int.from_bytes(s[5:9], "little") < 1 << 20 for _, s in ds)
        if codec == 16:
            assert all(X.size_field(s) < 1 << 20 for _, s in ds)
            heads = [fx.bases[d.base][1][0] for d, _ in ds]
            assert sum(bool(h & X.X_STRIPE) for h in heads) >= 50 and sum(bool(h & X.X_NOSZ) and not h & X.X_STRIPE for h in heads) >= 50
            assert all(d.op == X.OP_U16_TO for d, _ in ds if fx.bases[d.base][1][0] & X.X_NOSZ and not fx.bases[d.base][1][0] & X.X_STRIPE)
    # the inputs that are no vectors, and the old vectors
    assert len(re.findall(r"^\* no vector: ", text, flags=re.M)) == 4
    for word in ("N = 1 over 16,384 bytes", "N = 255 over 131 bytes", "in_size < N", "(4x8) over 0 bytes"):
        assert word in text, word
    assert "the reference reproduces 420 of its 420 entries" in text


def compress(oracle, orc8, c, order, data):
    return orc8.compress(data, order) if c.codec == 8 else oracle.compress(data, order)


def test_oracle_writes_every_reference_stream(oracle, orc8):
    for c in X.load().cases:
        data = X.case_input(c)
        for v in c.vectors:
            got = compress(oracle, orc8, c, v.order, data)
            assert got is not None, (c.name, v.order)
            assert (got if isinstance(v.stream, bytes) else X.digest(got)) == v.stream, (c.name, hex(v.order))


def test_oracle_decodes_every_reference_stream(oracle, orc8):
    for c in X.load().cases:
        data = X.case_input(c)
        for v in c.vectors:
            stream = v.stream if isinstance(v.stream, bytes) else compress(oracle, orc8, c, v.order, data)   # (held to the digest above)
            if c.codec == 8:
                assert orc8.uncompress(stream) == data, c.name
            else:
                assert oracle.uncompress(stream, capacity=len(data)) == data, (c.name, hex(v.order))
                if not stream[0] & X.X_NOSZ or stream[0] & X.X_STRIPE:
                    assert oracle.uncompress_malloc(stream) == data, (c.name, hex(v.order))
    # the base streams of the damage draw (not the ones put together by the maker, which stand in the draw unedited; a
    # stream without a size field is decoded at the capacity its damaged copies were handed over with, less the slack)
    fx = X.load()
    crafted = {d.base for d in fx.damaged if not d.edits}
    caps = {}
    for d in fx.damaged:
        if d.op == X.OP_U16_TO:
            caps[d.base] = min(caps.get(d.base, d.capacity), d.capacity)
    for k, (codec, stream) in enumerate(fx.bases):
        if k in crafted:
            continue
        if codec == 8:
            assert orc8.uncompress(stream) is not None, k
        elif stream[0] & X.X_NOSZ and not stream[0] & X.X_STRIPE:
            assert oracle.uncompress(stream, capacity=caps[k]) is not None, k
        else:
            assert oracle.uncompress_malloc(stream) is not None, k


@pytest.mark.parametrize("codec", (16, 8))
def test_stable_damaged_streams_get_the_reference_answer_or_fall_in_a_named_class(oracle, orc8, codec):
    bad, used = [], collections.Counter()
    for d, stream in X.damaged_streams(codec):
        if d.answer is None:
            oracle_answer(oracle, orc8, d.op, d.capacity, stream)                 # unstable: any answer, but an answer
            continue
        mine = oracle_answer(oracle, orc8, d.op, d.capacity, stream)
        why = judge(codec, stream, d.capacity, d.answer, mine)
        if why:
            bad.append(why)
        elif not same_answer(d.answer, mine):
            used.update(x.name for x in excused(codec, stream, d.capacity, d.answer, mine))
    assert not bad, bad[:10]
    print(dict(used))
    # a member of an entry is a stream whose bytes satisfy the predicate, whose answer from the reference is stable, and
    # on which the oracle really gives the other answer the entry names: every entry that is not the device's alone has one
    assert set(used) == {x.name for x in X.DEVIATIONS if x.codec == codec and x.what == "decode" and x.oracle != "follows"}, dict(used)


def test_every_deviation_has_a_member_in_the_fixture(oracle, orc8):
    """The entries that are the device's alone: each holds for a stream that the reference accepts stably, and there the
    oracle follows the reference (the device's own answer is tests/test_gpu_rans_edge.py's to hold).  The encoder's entry.
    And no reference-made stream of the encode cases satisfies any predicate."""
    seen = collections.Counter()
    for codec in (16, 8):
        for d, stream in X.damaged_streams(codec):
            hit = X.deviation(codec, stream, d.capacity)
            if d.answer not in (None, X.REFUSED) and hit and all(x.oracle == "follows" for x in hit):
                assert same_answer(d.answer, oracle_answer(oracle, orc8, d.op, d.capacity, stream)), stream[:24].hex()
                seen.update(x.name for x in hit)
    assert set(seen) == {x.name for x in X.DEVIATIONS if x.oracle == "follows"}, dict(seen)
    assert [x.name for x in X.deviation(8, b"", what="encode")] == ["x8_encode_nothing"] and orc8.compress(b"", 0) is None and orc8.compress(b"", 1) is None
    assert not X.deviation(8, b"a", what="encode")
    for c in X.load().cases:
        for v in c.vectors:
            if isinstance(v.stream, bytes):
                assert not X.deviation(c.codec, v.stream, len(X.case_input(c))), (c.name, hex(v.order))


def test_live_differential_against_the_reference(oracle, orc8):
    """1,000 random inputs of up to 70,000 bytes, each under a random flag set (4x16: bits 1 and 2 clear, stripes of 2 to 8
    planes; every fourth input goes to 4x8), through the reference - its sanitizers on - and the oracle: the same bytes.
    Then 2,000 damaged copies of those streams that are 30 to 1,500 bytes long, twice through the reference (runs A and
    B) and once through the oracle, judged as the fixture's are.  Host programs only: a machine without a reference tree
    has no driver, and this test is never one of the gpu ones."""
    if not os.path.exists(X.DRIVER):
        pytest.skip("no oracle/_ref/rans_ref: built by build() where a reference tree is")
    rng = random.Random(4242)
    recs = []
    for k in range(1000):
        data = X.random_input(rng, 70000 if k % 10 == 0 else 3000)
        if k % 4 == 3:
            recs.append((X.OP_C8, rng.randrange(2), 0, 0, data or b"x"))
        else:
            order = X.random_order(rng)
            if order >> 8 == 1 or (order & X.X_STRIPE and len(data) >= 16384 * (order >> 8)):
                order &= 0xff & ~X.X_STRIPE                                   # (no vector: README.edge.md)
            recs.append((X.OP_C16, order, 0, 0, data))
    res = X.run_driver(recs)
    bases = []
    for k, (rec, (answer, _, stream)) in enumerate(zip(recs, res)):
        assert answer == X.MADE, k
        codec = 8 if rec[0] == X.OP_C8 else 16
        mine = orc8.compress(rec[4], rec[1]) if codec == 8 else oracle.compress(rec[4], rec[1])
        assert mine == stream, (k, codec, hex(rec[1]), len(rec[4]))
        if 30 <= len(stream) <= 1500:
            bases.append((codec, rec, stream))
    assert len(bases) >= 300
    calls = []
    for k in range(2000):
        codec, rec, stream = bases[k % len(bases)]
        b = X.apply(stream, X.damage(rng, stream, codec))
        if codec == 8:
            calls.append((X.OP_U8, 0, b))
        elif stream[0] & X.X_NOSZ and not stream[0] & X.X_STRIPE or rng.random() < 0.5:
            calls.append((X.OP_U16_TO, len(rec[4]) + rng.choice((0, 64)), b))
        else:
            calls.append((X.OP_U16, 0, b))
    bad, stable, accepted = [], 0, 0
    for (op, cap, b), ref in zip(calls, X.answers_ab(calls)):
        if ref is None:
            continue
        stable += 1
        accepted += ref != X.REFUSED
        why = judge(8 if op == X.OP_U8 else 16, b, cap, ref, oracle_answer(oracle, orc8, op, cap, b))
        if why:
            bad.append(why)
    assert not bad, bad[:10]
    assert stable >= 1500 and accepted >= 500, (stable, accepted)
