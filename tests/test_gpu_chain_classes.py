"""The class tables of the chain launchers (htscodecs_amd/csrc/r4x16_decode.hip launch_dec_chain_of, r4x16_enc_chain.hip
r4x16_launch_enc_chain) where neither the residency table nor test_gpu_routes.py pins them:

  * the launch for nested order-1 tables (one_row_only): no route counter sees it, and a class skipped wrongly there
    leaves the table - and so the block - undecoded.  Order-1 blocks whose frequency table travels as an order-0
    stream, with that inner stream's alphabet in each range of the u16 rows' depths (<= 50, 51 .. 150, > 150 symbols);
  * order-0 payload streams: their own classes of two-read rows and of direct rows, and depths 3 and 4 on one-row images;
  * an order-0 and an order-1 stream with direct rows in one batch, the classes side by side and in stream order
    (which decides whether the order-0 stream has a class of its own);
  * the encoder's classes of order-0 streams: u16 rows and symbol records.

The streams are the CPU oracle's; decoded bytes are compared with the raw input, encoded bytes with the oracle's."""
import numpy as np
import pytest

import datagen
from test_gpu_dec_step import _alphabet_of, _varint, stream_info
from test_gpu_routes import _dev_decode, _dev_encode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd


def _codec(H, **options):
    dc = H.DeviceCodec(0)
    dc.set_option("route_count", 1)
    for k, v in options.items():
        dc.set_option(k, v)
    return dc


def _routes(dc, which="decode"):
    return {k: v for k, v in dc.route_read(which).items() if v}


# ---- nested tables ---------------------------------------------------------------------------------------------------
def _skewed(n, values, seed):
    """n i.i.d. bytes over `values`, the symbol probabilities one draw from Dirichlet(0.3)."""
    rs = np.random.RandomState(seed)
    p = rs.dirichlet([0.3] * len(values))
    return np.asarray(values, dtype=np.uint8)[rs.choice(len(values), size=n, p=p)]


def _inner_alphabet(comp):
    """Symbols of the order-0 stream that carries the table of an order-1 block (it starts with its alphabet)."""
    assert comp[0] == 1, "not a plain order-1 block"
    _, pos = _varint(comp, 1)
    assert comp[pos] & 1, "the table is not an order-0 stream"
    _, pos = _varint(comp, pos + 1)                        # the table's size
    _, pos = _varint(comp, pos)                            # the inner stream's size
    return len(_alphabet_of(comp, pos)[0])


NESTED = {                                                  # name: (input, range of the inner alphabet)
    "depth2": (lambda: datagen.rand(70000, 1, 40, 33), range(1, 51)),
    "depth3": (lambda: _skewed(70000, np.arange(33, 73), 1), range(51, 151)),
    "depth4": (lambda: _skewed(200000, np.arange(0, 256, 2), 1), range(151, 257)),
}


@pytest.fixture(scope="module")
def nested(oracle):
    out = {}
    for name, (make, rng) in NESTED.items():
        raw = make().tobytes()
        comp = oracle.compress(raw, 1)
        assert _inner_alphabet(comp) in rng, (name, _inner_alphabet(comp))
        out[name] = (raw, comp)
    return out


@pytest.mark.parametrize("direct", [1, 0])
@pytest.mark.parametrize("which", list(NESTED) + ["all"])
def test_nested_tables_of_every_depth(H, nested, which, direct):
    dc = _codec(H, dec_direct=direct)
    names = list(NESTED) if which == "all" else [which]
    got = _dev_decode(dc, [nested[n][1] for n in names], [len(nested[n][0]) for n in names])      # (asserts status 0)
    assert [g == nested[n][0] for g, n in zip(got, names)] == [True] * len(names), (which, direct)


# ---- order-0 payload streams -----------------------------------------------------------------------------------------
O0_NSYM = (50, 51, 150, 151, 256)
O0_ROUTE = {0: ("l2", "l3", "l3", "l4", "l4"),            # u16 rows by depth
            1: ("direct", "direct", "l3", "l4", "l4")}    # direct rows up to 128 symbols


@pytest.fixture(scope="module")
def order0(oracle):
    out = {}
    for ns in O0_NSYM:
        raw = datagen.weighted(70000, np.linspace(1, 8, ns), ns).tobytes()
        comp = oracle.compress(raw, 0)
        info = stream_info(comp)
        assert info.coded and info.order == 0 and info.nsym == ns, (ns, info)
        out[ns] = (raw, comp)
    return out


@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("ns", O0_NSYM)
def test_order0_streams_land_on_their_class(H, order0, ns, direct):
    raw, comp = order0[ns]
    dc = _codec(H, dec_direct=direct)
    dc.route_read("decode")
    assert _dev_decode(dc, [comp], [len(raw)]) == [raw]
    assert _routes(dc) == {O0_ROUTE[direct][O0_NSYM.index(ns)]: 1}, (ns, direct)


@pytest.mark.parametrize("direct,kind", [(0, "u16"), (1, "records")])
@pytest.mark.parametrize("ns", O0_NSYM)
def test_order0_streams_encode_on_their_class(H, order0, ns, direct, kind):
    raw, comp = order0[ns]
    dc = _codec(H, enc_direct=direct)
    dc.route_read("encode")
    assert _dev_encode(dc, [np.frombuffer(raw, dtype=np.uint8)], 0) == [comp]
    assert _routes(dc, "encode") == {kind: 1}, (ns, direct)


# ---- both orders with direct rows in one batch -----------------------------------------------------------------------
@pytest.mark.parametrize("concurrent", [1, 0])
def test_direct_rows_of_both_orders_in_one_batch(H, oracle, concurrent):
    raws = [datagen.tile("q8", 65536, 0).tobytes(), datagen.tile("q40+dir", 65536, 0).tobytes()]
    comps = [oracle.compress(r, order) for r, order in zip(raws, (0, 1))]
    assert [stream_info(c).order for c in comps] == [0, 1] and all(stream_info(c).coded for c in comps)
    dc = _codec(H, dec_direct=1, sched_concurrent=concurrent)
    dc.route_read("decode")
    assert _dev_decode(dc, comps, [len(r) for r in raws]) == raws
    assert _routes(dc) == {"direct": 2}, concurrent
