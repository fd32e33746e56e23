"""The decode chain on packed rows of layout 2 (htscodecs_amd/csrc/r4x16_decode.hip: chain_decode_pk2) where the deferred
tail of its 16-step trips can go wrong.  A trip's store, the flags of its last row, the loop test's operands and the
refill of a lane that is one quarter on stand in the group-read shadows of the NEXT trip; a lane two quarters on takes
the immediate refill behind the body; whatever is still open when the loop ends is done in an epilogue.

  1. 46 and 13 symbols, 15 streams, 4,032, 4,092, 4,096, 4,100, 4,156 and 4,099 bytes: the chains' counts are 16n, 16n - 1,
     16n, 16n + 1, 16n + 15 and (three chains) 16n with one of 16n + 3, so the loop ends with each kind of work still open
     (a store, a store and a refill, flags of a row that the next step does or does not use);
  2. 1, 7 and 15 streams: idle lanes run under the in-body exec masks and must neither store, write the ring nor ask;
  3. fifteen streams of unequal length, 4,096 to 65,537 bytes, unsorted, in one wave: the wave leaves the 16-step trips
     while others have work open;
  4. the stream that crosses two quarters in one trip at each of the 16 alignments beside 14 slower ones: the immediate
     refill and the deferred one in one wave;
  5. the quarter stream that makes its wave leave the 16-step trips early;
  6. the stream without words among ordinary ones and at both edges of the allocation (the deferred request is the
     unconditional one of `request`);
  7. the hostile stream that enters a context without a table behind trips of sixteen (ST_CONTEXT: the deferred flags).

Streams are made by the CPU oracle with the generators of test_gpu_dec_refill.py, test_gpu_dec_trip16.py and
test_gpu_dec_shadow.py; the decoded bytes are compared with the RAW INPUT between guard bytes, no stray write, the input
arena unchanged (decode() of test_gpu_dec_step.py asserts both), and every case asserts its route as l1."""
import functools

import pytest

import test_gpu_dec_refill as R
import test_gpu_dec_shadow as S
from test_gpu_dec_step import H, device, stream_info  # noqa: F401
from test_gpu_dec_trip16 import ENTRY_WORDS, PAD

SIZES = (4032, 4092, 4096, 4100, 4156, 4099)
UNEQUAL = (4096, 4099, 5000, 6001, 8192, 9000, 12289, 16384, 20000, 24577, 32768, 40001, 49152, 60000, 65537)
WAVE = R.WAVE
OPTS = S.OPTS


def counts(size):
    """steps of the four chains of a stream of `size` bytes"""
    q = size >> 2
    return [q, q, q, q + size - 4 * q]


@functools.lru_cache(maxsize=None)
def wave_of(n, size):
    return [R.long_stream(n, i, size) for i in range(WAVE)]


@functools.lru_cache(maxsize=None)
def unequal():
    return [R.long_stream(46, i, length) for i, length in enumerate(UNEQUAL)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("n", (46, 13))
def test_loop_ends_with_each_kind_of_work_open(H, opts, n, size):
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    R.run(dc, wave_of(n, size), shifts=[(3 * i + n) % 16 for i in range(WAVE)])


@pytest.mark.gpu
@pytest.mark.parametrize("streams", (1, 7, 15))
@pytest.mark.parametrize("n", (46, 13))
def test_idle_lanes_under_the_in_body_masks(H, opts, n, streams):
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    R.run(dc, wave_of(n, 4100)[:streams], shifts=[(7 * i + 2) % 16 for i in range(streams)])


@pytest.mark.gpu
def test_unequal_lengths_in_one_wave(H, opts):
    dc = device(H, opts, dict(OPTS, sched_sort=0))
    R.run(dc, unequal(), shifts=[(5 * i + 3) % 16 for i in range(WAVE)])


@pytest.mark.gpu
def test_immediate_and_deferred_refill_in_one_wave(H, opts):
    R.test_two_quarter_crossing_at_every_alignment(H, opts)


@pytest.mark.gpu
def test_quarter_stream(H, opts):
    R.test_quarter_stream_leaves_the_sixteen_step_trips_early(H, opts)


@pytest.mark.gpu
@pytest.mark.parametrize("place", (0, 14))
def test_stream_without_words_among_ordinary_ones(H, opts, place):
    R.test_stream_without_words_among_ordinary_ones(H, opts, place)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ("first", "last"))
def test_stream_without_words_at_the_edge_of_the_allocation(H, opts, where):
    R.test_stream_without_words_at_the_edge_of_the_allocation(H, opts, where)


@pytest.mark.gpu
def test_context_without_a_table_with_deferred_flags(H, opts):
    R.test_context_without_a_table_behind_trips_of_sixteen(H, opts)


# ---- CPU: the cases are what they claim --------------------------------------------------------------------------
def test_cases_are_what_they_claim():
    from test_gpu_routes import _expected_level
    assert [c % 16 for c in counts(4032)] == [0, 0, 0, 0] and [c % 16 for c in counts(4092)] == [15] * 4
    assert [c % 16 for c in counts(4096)] == [0] * 4 and [c % 16 for c in counts(4100)] == [1] * 4
    assert [c % 16 for c in counts(4156)] == [15] * 4 and [c % 16 for c in counts(4099)] == [0, 0, 0, 3]
    assert counts(4092)[0] == 16 * 64 - 1 and counts(4156)[0] == 16 * 64 + 15
    for n in (46, 13):
        assert _expected_level(n, 0, 0) == "l1"
        for size in SIZES:
            for name, raw, s in wave_of(n, size):
                info = stream_info(s)
                assert info.coded and info.order == 1 and info.bits == 10 and info.nsym == n, (name, info)
                assert len(raw) == size and info.nwords - PAD // 2 >= 4 * ENTRY_WORDS, name
    assert UNEQUAL[0] == 4096 and UNEQUAL[-1] == 65537 and len(UNEQUAL) == WAVE
    for (name, raw, s), length in zip(unequal(), UNEQUAL):
        info = stream_info(s)
        assert info.coded and info.order == 1 and info.nsym == 46 and len(raw) == length, (name, info)
