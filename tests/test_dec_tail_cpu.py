"""No GPU.  An integer model of the ring of the decode chain's 16-step trips under the DEFERRED schedule
(htscodecs_amd/csrc/r4x16_decode.hip: chain_decode_pk2), beside the model of the immediate refill in
tests/test_dec_refill_cpu.py (`New`).

The schedule: at a trip's end a lane is 0, 1 or 2 quarters on.  Two quarters on (in any lane of the wave; the model is one
stream) is the fallback: the immediate refill, both rounds, behind the body.  One quarter on is deferred: the park, the
mirror write and the request of the immediate refill's one round are done in a group-read shadow of the NEXT trip, and so
is the trip's store, behind them.  Shadow u (1 .. 16) of a trip follows the ring read of the trip's step u (steps 0 .. 15;
step 16 is the next trip's step 0, whose read is issued in shadow 16): work deferred to shadow u is seen by the reads of
steps u + 1 onwards.  The device uses shadows 6 and 7 for the two parities and 8 for the store.

The bound.  A lane one quarter on has its cursor below the end of stream quarter half + 1, and slot `half` is next needed
for stream quarter half + 4, 128 bytes further.  A step moves the cursor by at most 8 bytes and reads 12 from the cursor
rounded DOWN to four: the read of step j ends at or below (end - 1 + 8 j) & ~3) + 12, which is the end of quarter half + 3
for j = 15 and beyond it for j = 16.  By the coarser count without the rounding (8 j + 12 <= 128) shadows up to 14 are
safe; the sweep below asserts every shadow up to 14, finds 15 still safe by the exact count and shadow 16 the first that
fails, on the walk that takes 8 bytes in every step from the last byte of a quarter."""
import copy

import numpy as np
import pytest

from test_dec_refill_cpu import RB, TRIP, New, Stream

PARK_SHADOW = (7, 6)            # by the parity of `half`: even, odd
STORE_SHADOW = 8


class Deferred(New):
    """The ring under the deferred schedule.  `shadow`: where the deferred refill is done (None: the device's two)."""

    def __init__(self, st, shadow=None):
        New.__init__(self, st)
        self.shadow, self.open_refill, self.open_store, self.stored, self.fallbacks = shadow, False, None, [], 0

    def end_of_trip(self, trip, nh):
        """behind the body: nothing is open but this trip's own refill and store"""
        assert not self.open_refill and self.open_store is None
        on = nh - self.half
        assert 0 <= on <= 2
        if on == 2:
            self.fallbacks += 1
            self.refill(nh)                                  # the immediate refill, both rounds
        else:
            self.open_refill = on == 1
        self.open_store = trip
        return on

    def in_shadow(self, u):
        """the deferred work of shadow u of the trip that follows"""
        at = self.shadow if self.shadow is not None else PARK_SHADOW[self.half & 1]
        if self.open_refill and u == at:
            self.refill(self.half + 1)                       # one round: park, mirror or pad, request
            self.open_refill = False
        if self.open_store is not None and u == max(STORE_SHADOW, at + 1 if self.shadow is not None else STORE_SHADOW):
            assert not self.open_refill, "the store stands behind the refill"
            self.stored.append(self.open_store)
            self.open_store = None

    def epilogue(self, nh):
        """the loop ends: the immediate refill for whatever is open, then the store"""
        if self.open_refill:
            self.refill(nh)
            self.open_refill = False
        if self.open_store is not None:
            self.stored.append(self.open_store)
            self.open_store = None


def same_state(imm, dfr, stored):
    assert imm.half == dfr.half
    assert imm.asked == dfr.asked, "the same chunks, in the same order"
    assert np.array_equal(imm.ring[:RB + 8], dfr.ring[:RB + 8]), "the ring and its mirror"
    for a, b in zip(imm.pend, dfr.pend):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "the waiting quarters"
    assert dfr.stored == stored, "every trip's bytes stored once, in order"


def walk(rng, off0, words_len, take, shadow=None):
    """One stream through the 16-step trips under both schedules.  `take(trip, step)`: words the quad takes in a step,
    0 .. 4.  Every read's window must hold the stream's bytes; from the shadow that does the deferred refill to the
    trip's end the ring equals the immediate model's; leaving the loop after ANY trip hands over the immediate model's
    state.  Returns the quarters-on seen at trip ends and whether a request was clamped."""
    st = Stream(rng, off0, words_len)
    imm, dfr = New(st), Deferred(st, shadow)
    nwords, cursor, seen, trip, stored = words_len >> 1, 0, [], 0, []
    while cursor + 64 <= nwords:
        for j in range(TRIP):
            # the ring read of step j, then shadow j (shadow 0 is the trip before's sixteenth: nothing deferred stands there)
            cb = off0 + 2 * cursor
            ra = cb & (RB - 4)
            got, want = dfr.ring[ra:ra + 12], st.aligned[cb & ~3:(cb & ~3) + 12]      # (short at the stream's very end)
            assert np.array_equal(got[:len(want)], want), ("window", off0, words_len, trip, j)
            assert np.array_equal(got, imm.ring[ra:ra + 12])
            if j:
                dfr.in_shadow(j)
            if not dfr.open_refill:
                assert np.array_equal(imm.ring[:RB + 8], dfr.ring[:RB + 8]), (trip, j)
            n = take(trip, j)
            assert 0 <= n <= 4
            cursor += n
        # shadow 16 follows the read of the next trip's step 0: modelled by the caller's sweep only (in_shadow(16) below)
        nh = (off0 + 2 * cursor) >> 6
        if dfr.open_refill or dfr.open_store is not None:    # a sweep beyond shadow 15: the work is still open at the trip's end
            cb = off0 + 2 * cursor
            ra = cb & (RB - 4)
            want = st.aligned[cb & ~3:(cb & ~3) + 12]
            assert np.array_equal(dfr.ring[ra:ra + len(want)], want), ("window", off0, words_len, trip, 16)
            dfr.in_shadow(16)
        on = nh - imm.half
        imm.refill(nh)
        stored.append(trip)
        assert dfr.end_of_trip(trip, nh) == on
        assert (dfr.fallbacks > 0) == (2 in seen + [on]) and dfr.fallbacks == (seen + [on]).count(2), "the fallback fires exactly at two quarters on"
        seen.append(on)
        # leaving the loop here, with a refill and a store open or not
        out = copy.deepcopy(dfr)
        out.epilogue(nh)
        same_state(imm, out, stored)
        trip += 1
    return seen, any(c == st.lastc for c in dfr.asked[24:])


def random_take(rng, rate):
    return lambda trip, j: int((rng.random(4) < rate).sum())


WALKS = ((0.05, 700), (0.45, 3000), (0.98, 4000), (1.0, 2 * 64 + 2 * 37), (0.7, 1234), (0.3, 130), (1.0, 4096))


@pytest.mark.parametrize("off0", range(16))
def test_deferred_schedule_against_the_immediate_one(off0):
    rng = np.random.default_rng(500 + off0)
    seen, clamp, open_at_exit = set(), False, set()
    for rate, words_len in WALKS:
        s, c = walk(rng, off0, words_len, random_take(rng, rate))
        seen |= set(s)
        clamp |= c
        open_at_exit |= set(s[-1:])
    assert seen == {0, 1, 2}, (off0, seen)                    # nothing, the deferred refill, the fallback
    assert clamp, "lastc reached in the middle of a walk"
    assert 1 in seen


def test_whole_trips_at_eight_bytes_a_step():
    rng = np.random.default_rng(600)
    for off0 in range(16):
        seen, _ = walk(rng, off0, 8192, lambda trip, j: 4)
        assert set(seen) == {2}, "128 bytes a trip: two quarters on at every trip's end"
        # alternating 4 and 0 words: 64 bytes a trip, one quarter on at every trip's end, all of it deferred
        seen, _ = walk(rng, off0, 8192, lambda trip, j: 4 * (j & 1))
        assert set(seen) == {1}


def test_a_stream_without_words_never_enters_the_trips():
    rng = np.random.default_rng(601)
    seen, _ = walk(rng, 0, 0, lambda trip, j: 0)
    assert seen == []
    st = Stream(rng, 0, 0)
    d = Deferred(st)
    assert np.array_equal(d.request(64 * 7 + 384), st.front) and d.asked == []


def worst_walk(off0, shadow):
    """the cursor on the last byte of a quarter at a trip's end, one quarter on, then 8 bytes in every step"""
    rng = np.random.default_rng(602)
    # trip 0 brings cb from off0 to 127 (off0 odd) or 126: one quarter on, the deferred case; then 4 words a step
    want = (127 - off0) // 2

    def take(trip, j):
        if trip == 0:
            return min(4, max(0, want - 4 * j))
        return 4
    return walk(rng, off0, 2048, take, shadow)


@pytest.mark.parametrize("shadow", range(1, 17))
def test_sweep_of_the_deferral_step(shadow):
    """Safe in every shadow up to 14 (the bound), still safe in 15 by the exact count, and the window of the next trip's
    first step, read in front of shadow 16, is the first that misses its quarter: the bound is exercised."""
    if shadow <= 15:
        for off0 in range(16):
            seen, _ = worst_walk(off0, shadow)
            assert seen[0] == 1
            if off0 in (0, 7, 15):
                rng = np.random.default_rng(700 + shadow)
                for rate, words_len in WALKS:
                    walk(rng, off0, words_len, random_take(rng, rate), shadow)
    else:
        with pytest.raises(AssertionError, match="window"):
            worst_walk(15, shadow)
