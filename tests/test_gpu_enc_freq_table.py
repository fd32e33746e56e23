"""The encoder's packed rows in their two kinds (htscodecs_amd/csrc/r4x16_common.h): blocks whose highest byte is below
128 take the image with the 128-byte index and are coded from the 8-byte frequency table (route kind "packed_freq",
EncOutT::step_freq); blocks that reach byte 128 keep the 256-byte index and the step that derives shift and complement
from the frequency.  Both must give the oracle's bytes, at the edges of the index (highest byte 127 / 128), at the
frequencies where the two steps differ in how they divide (1, 2, 3, 1024), at every length modulo four and below one
double trip of the pipelined loop, and side by side in one batch.  Every case asserts the route it ran on.

What the inputs are made to contain is checked on the CPU, from the oracle's own table bytes, by
test_inputs_hold_what_they_claim - which needs no GPU."""
import numpy as np
import pytest


# ---- inputs ------------------------------------------------------------------------------------------------------------

def _plain(alpha, n, seed):
    """n bytes drawn evenly from `alpha` (byte values)."""
    a = np.asarray(alpha, dtype=np.uint8)
    return a[np.random.RandomState(seed).randint(0, len(a), size=n)]


def _special(alpha, n, seed):
    """n bytes over `alpha` with two made-up context rows.  The last byte value of `alpha` is only ever followed by the
    first one: its row holds one symbol, frequency 1024 after normalisation.  The last but one occurs exactly 2,048 times
    as a context and is followed once, four and six times by three values that occur nowhere else, and by one common
    value otherwise: the normalisation to 1,024 (which rounds down, and never to zero) makes that the frequencies 1, 2
    and 3 - checked against the oracle's table below, not taken on trust."""
    a = np.asarray(alpha, dtype=np.uint8)
    rs = np.random.RandomState(seed)
    common = a[:-5]
    single, ctx, x3, x2, x1 = a[-1], a[-2], a[-3], a[-4], a[-5]
    pairs = [(single, common[0])] * 40 + [(ctx, x1)] + [(ctx, x2)] * 4 + [(ctx, x3)] * 6 + [(ctx, common[1])] * 2037
    rs.shuffle(pairs)
    fill = n - 2 * len(pairs)
    assert fill >= 4 * len(pairs), "room for a common byte on both sides of every pair"
    # a pair, then a run of common bytes (at least two): no pair touches another one
    runs = np.full(len(pairs), 2, dtype=np.int64)
    extra = rs.multinomial(fill - 2 * len(pairs) - 64, np.ones(len(pairs)) / len(pairs))
    out = [common[rs.randint(0, len(common), size=64)]]                 # the block starts with common bytes
    for p, r in zip(pairs, runs + extra):
        out.append(np.array(p, dtype=np.uint8))
        out.append(common[rs.randint(0, len(common), size=int(r))])
    d = np.concatenate(out)
    assert len(d) == n
    return d


LOW46 = list(range(33, 78))                   # 45 byte values and byte 0: a 46-symbol alphabet inside 0..127
STRADDLE46 = list(range(106, 151))            # the same size across 128
TOP127 = list(range(100, 128))                # highest byte 127: the last one the short index holds
TOP128 = list(range(101, 129))                # highest byte 128: the first one it does not
SMALL_LOW = list(range(40, 64))               # 24 values for the made-up rows (a table short enough to travel as it is)
SMALL_HIGH = list(range(140, 164))


def _cases():
    """name -> (bytes, short index expected)."""
    c = {}
    for k in range(4):                                                   # lengths 4 q + {0, 1, 2, 3}
        c[f"low46-4q+{k}"] = (_plain(LOW46, 40000 + k, 10 + k), True)
        c[f"straddle46-4q+{k}"] = (_plain(STRADDLE46, 40000 + k, 20 + k), False)
        c[f"rows-low-4q+{k}"] = (_special(SMALL_LOW, 16000 + k, 30 + k), True)
        c[f"rows-high-4q+{k}"] = (_special(SMALL_HIGH, 16000 + k, 40 + k), False)
    c["top127"] = (_plain(TOP127, 30001, 50), True)
    c["top128"] = (_plain(TOP128, 30001, 51), False)
    for name, alpha, short in (("low", SMALL_LOW, True), ("high", SMALL_HIGH, False)):
        a = np.asarray(alpha, dtype=np.uint8)
        # below one double trip of the pipelined loop (eight steps a chain: q - 1 < 8) and just above it: every value of
        # the alphabet once, then more of them.  Twenty symbols in so few bytes never code smaller than they are: the
        # container holds them raw - after the chain has coded them, for its length decides that (rANS_static4x16pr.c:1332)
        for n in (24, 27, 32, 35, 36, 37, 38, 39, 43, 71):
            c[f"short-{name}-{n}"] = (np.concatenate([a, _plain(alpha, n - len(a), n)]), short)
        # the shortest blocks that do go out coded: the alphabet once, then one value over and over (a few double trips)
        for n in (150, 151, 152, 153):
            c[f"brief-{name}-{n}"] = (np.concatenate([a, np.full(n - len(a), a[3], dtype=np.uint8)]), short)
    return c


CASES = _cases()


# ---- the oracle's table, read back ---------------------------------------------------------------------------------------

def _varint(b, i):
    v = 0
    while True:
        c = b[i]
        i += 1
        v = (v << 7) | (c & 0x7f)
        if not c & 0x80:
            return v, i


def _table(comp):
    """(bits, {context byte: {byte: frequency as the coder uses it}}) of an order-1 container without transforms whose
    table travels uncompressed; (bits, None) where the table is itself a compressed stream."""
    assert comp[0] == 1, "a plain order-1 container"
    _, i = _varint(comp, 1)
    bits, nested = comp[i] >> 4, comp[i] & 1
    i += 1
    if nested:
        return bits, None
    # the alphabet: values in ascending order, a run of consecutive ones as (first, second, count of further ones)
    alpha, rle, j = [], 0, comp[i]
    i += 1
    while True:
        alpha.append(j)
        if not rle and j + 1 == comp[i]:
            j, rle = comp[i], comp[i + 1]
            i += 2
        elif rle:
            rle -= 1
            j += 1
        else:
            j = comp[i]
            i += 1
        if j == 0:
            break
    rows = {}
    for r in alpha:
        row, run = {}, 0
        for s in alpha:
            if run:
                run -= 1
                continue
            f, i = _varint(comp, i)
            if f == 0:
                run = comp[i]
                i += 1
            else:
                row[s] = f
        tot = sum(row.values())
        if tot:
            sh = 0
            while (tot << sh) < (1 << bits):
                sh += 1
            assert (tot << sh) == (1 << bits), (r, tot)
            rows[r] = {s: f << sh for s, f in row.items()}
    return bits, rows


def _nsym(a):
    return len(set(np.unique(a).tolist()) | {0})


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_hold_what_they_claim(oracle, name):
    """The oracle alone: every case is a 10-bit order-1 table of 20..64 symbols (what the packed rows take), round-trips,
    has its highest byte on the side of 128 it stands for - and the made-up rows hold the frequencies 1, 2, 3 and 1024."""
    data, short = CASES[name]
    raw = data.tobytes()
    comp = oracle.compress(raw, 1)
    assert oracle.uncompress(comp, len(raw)) == raw
    if name.startswith("short-"):
        assert comp[0] == 0x20 and comp[-len(raw):] == raw, "stored raw"
        rows = None
    else:
        bits, rows = _table(comp)
        assert bits == 10, (name, bits)
    assert 20 <= _nsym(data) <= 64, (name, _nsym(data))
    assert (int(data.max()) < 128) == short
    if name == "top127":
        assert int(data.max()) == 127
    if name == "top128":
        assert int(data.max()) == 128
    if name.startswith(("low46", "straddle46")):
        assert _nsym(data) == 46
        assert name.startswith("low46") or (int(data.min()) < 128 <= int(data.max()))
    if name.startswith("rows-"):
        assert rows is not None, "the table of this case must travel uncompressed to be read back"
        a = SMALL_LOW if short else SMALL_HIGH
        single, ctx, x3, x2, x1 = a[-1], a[-2], a[-3], a[-4], a[-5]
        assert rows[single] == {a[0]: 1024}, rows[single]
        assert rows[ctx][x1] == 1 and rows[ctx][x2] == 2 and rows[ctx][x3] == 3 and sum(rows[ctx].values()) == 1024, rows[ctx]
    if "4q+" in name:
        assert len(raw) % 4 == int(name[-1])


# ---- on the GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd


def _run(H, oracle, opts, names):
    """The cases `names` as ONE single-pass host batch on the full chip's rows (no symbol records): the oracle's bytes
    both ways, and the route read-out of the encode chain."""
    from htscodecs_amd import codec
    opts.set("route_count", 1)
    opts.set("enc_direct", 0)
    opts.set("host_pipe_mb", 0)
    raws = [CASES[n][0].tobytes() for n in names]
    want = [oracle.compress(r, 1) for r in raws]
    codec.route_read("encode")
    enc, st = H.compress_batch(raws, [1] * len(raws))
    assert all(s == 0 for s in st), st
    route = codec.route_read("encode")
    bad = [n for n, e, w in zip(names, enc, want) if e != w]
    assert not bad, bad
    dec, st = H.uncompress_batch(want, [len(r) for r in raws])
    assert all(s == 0 for s in st), st
    assert dec == raws
    return route


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_each_case_alone(H, oracle, opts, name):
    route = _run(H, oracle, opts, [name])
    assert route["records"] == 0 and route["packed"] == 1, route
    assert route["packed_freq"] == (1 if CASES[name][1] else 0), route


@pytest.mark.gpu
def test_both_kinds_side_by_side(H, oracle, opts):
    """Every case in one batch, the two kinds interleaved: both classes are launched for the same call."""
    names = sorted(CASES, key=lambda n: n[::-1])
    nshort = sum(1 for n in names if CASES[n][1])
    assert 0 < nshort < len(names)
    route = _run(H, oracle, opts, names)
    assert route["records"] == 0 and route["packed"] == len(names), route
    assert route["packed_freq"] == nshort, route


@pytest.mark.gpu
def test_quality_alphabet_keeps_45_streams_per_cu(H):
    dc = H.DeviceCodec(0)
    assert dc.residency(False, 46, 1, 10)[0] == 45
