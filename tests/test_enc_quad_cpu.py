"""The quad's emit count of the encode chain's packed-row step (htscodecs_amd/csrc/r4x16_enc_chain.h: ENC_TRIP_STEP,
EncOutT::trip_enter / trip_leave, flush_pipelined<true>) as an integer model, against emit16q's arithmetic.  No GPU.

emit16q (the C++ form, which phases A, B' and C still run): with m the wave's 64-bit mask of lanes over x_max,
    em = m >> (lane & ~3);  j = written + popc(em & above);  slot = emit ? j & 63 : -1;  written += popc(em & 15)
The statement: two lane constants made once, mlo / mhi = (above | 1 << k) << (lane & 28) in the half of the wave the quad
lies in and 0 in the other, and per step
    t = wm1 + popc((m_lo & mlo) | (m_hi & mhi));  slot = emit ? t & 63 : -1;  wm1 = t of the quad's lane 0
with wm1 = written - 1 (mod 2^32, so 0xffffffff at a stream's start).  Everything is 32-bit arithmetic as the
instructions do it (v_and_b32, v_and_or_b32, v_bcnt_u32_b32 with accumulate, v_mov_b32_dpp quad_perm 0,0,0,0,
v_and_b32 63, v_cndmask_b32, v_mad_i32_i24)."""
import itertools

import numpy as np
import pytest

M32 = 0xffffffff
QUADS = (0, 28, 32, 60)                  # first lanes: the ends of both halves of the wave
RING126 = 0x3e7e                         # an LDS address of a ring's last word slot (any 16-bit value does)


def popc(v):
    return bin(v).count("1")


def above_of(k):
    return (0xe << k) & 0xf              # the quad's lanes that write before lane k: chains k + 1 .. 3


# ---- the parent's arithmetic: emit16q<true>
def old_step(m, lane, written):
    """(slot or -1, ring address, written behind the step) of one lane"""
    k = lane & 3
    em = (m >> (lane & ~3)) & M32
    emit = (m >> lane) & 1
    j = (written + popc(em & above_of(k))) & M32
    slot = (j & 63) if emit else -1
    return slot, RING126 - 2 * slot, (written + popc(em & 0xf)) & M32


# ---- the statement's arithmetic
def masks(lane):
    k = lane & 3
    aos = ((above_of(k) | 1 << k) << (lane & 28)) & M32
    return (aos, 0) if lane < 32 else (0, aos)


def new_t(m, lane, wm1):
    mlo, mhi = masks(lane)
    t = (m & M32) & mlo                                  # v_and_b32     t, vcc_lo, mlo
    t = ((m >> 32) & mhi) | t                            # v_and_or_b32  t, vcc_hi, mhi, t
    return (popc(t) + wm1) & M32                         # v_bcnt_u32_b32 t, t, wm1


def new_step(m, lane, wm1):
    """(slot or -1, ring address, wm1 behind the step) of one lane; wm1 comes from the quad's lane 0"""
    t = new_t(m, lane, wm1)
    emit = (m >> lane) & 1
    slot = (t & 63) if emit else -1                      # v_and_b32 63; v_cndmask_b32 -1, t, vcc
    return slot, RING126 - 2 * slot, new_t(m, lane & ~3, wm1)        # v_mad_i32_i24 slot, -2, ring126; the DPP move


def neighbours(q0, rng, n):
    """masks of the OTHER quads of the wave: none, all, every lane but the quad's neighbours', and random ones"""
    own = 0xf << q0
    fixed = [0, ~own & (2 ** 64 - 1), (0xf << ((q0 + 4) % 64)), (0xf << ((q0 - 4) % 64)), 1 << ((q0 + 32) % 64),
             0xffffffff << (0 if q0 >= 32 else 32)]
    return [f & ~own for f in fixed] + [(int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2))) & ~own for _ in range(n)]


def test_lane_constants():
    """One of the two masks is 0, the other holds this lane and the lanes before it at the quad's place in its half."""
    for lane in range(64):
        mlo, mhi = masks(lane)
        k, q0 = lane & 3, lane & ~3
        full = mlo | mhi << 32
        assert (mlo == 0) != (mhi == 0) and (mlo == 0) == (lane >= 32)
        assert full == sum(1 << (q0 + i) for i in range(k, 4))
        assert full & ~(0xf << q0) == 0                     # nothing outside the quad
    assert masks(0)[0] == 15 and masks(3)[0] == 8 and masks(60)[1] == 0xf0000000 and masks(35)[1] == 8


@pytest.mark.parametrize("q0", QUADS)
def test_every_pattern_every_lane(q0):
    """All sixteen emit patterns of the quad, every k, `written` at its start value, around the ring's wrap at 64 and at
    large values, the rest of the wave emitting anything: slot, address and the carried count equal emit16q's, and a
    neighbour's bits change nothing."""
    rng = np.random.default_rng(q0 + 1)
    others = neighbours(q0, rng, 24)
    for pat, written in itertools.product(range(16), [0, 1, 2, 3, 4, 31, 32, 33, 59, 60, 61, 62, 63, 64, 65, 66, 127, 128, 524287, 2 ** 31 - 2]):
        wm1 = (written - 1) & M32
        first = None
        for o in others:
            m = pat << q0 | o
            got = []
            for k in range(4):
                lane = q0 + k
                s_old, a_old, w_old = old_step(m, lane, written)
                s_new, a_new, wm1_new = new_step(m, lane, wm1)
                assert (s_new, a_new) == (s_old, a_old), (pat, written, k, hex(o))
                assert (wm1_new + 1) & M32 == w_old, (pat, written, k, hex(o))
                got.append((s_new, wm1_new))
            assert len({w for _, w in got}) == 1                  # the four lanes carry the same count
            if first is None:
                first = got
            assert got == first, (pat, written, hex(o))            # independent of every other quad
        # the slots of a step: the emitting lanes, from chain 3 down, take consecutive words behind the last one written
        want = written
        for k in (3, 2, 1, 0):
            if pat >> k & 1:
                assert first[k][0] == want & 63
                want += 1
            else:
                assert first[k][0] == -1
        assert (first[0][1] + 1) & M32 == want & M32


def test_start_value_and_ring_wrap():
    """wm1 starts at 0xffffffff: the first word goes to slot 0.  A stream of steps that emit 0 .. 4 words walks the ring
    round several times; both forms place every word alike, and wm1 + 1 is `written` after every step."""
    assert new_step(0xf, 3, M32)[0] == 0 and new_step(0xf, 0, M32)[0] == 3 and new_step(0xf, 0, M32)[2] == 3
    assert new_step(0x1, 0, M32) == (0, RING126, 0) and new_step(0, 0, M32) == (-1, RING126 + 2, M32)
    rng = np.random.default_rng(5)
    for q0 in QUADS:
        written, wm1, ring_old, ring_new = 0, M32, {}, {}
        for step in range(400):
            m = int(rng.integers(0, 16)) << q0 | (int(rng.integers(0, 2 ** 63)) * 2 & ~(0xf << q0))
            for k in range(4):
                s_old, _, w2 = old_step(m, q0 + k, written)
                s_new, _, wm2 = new_step(m, q0 + k, wm1)
                if s_old >= 0:
                    ring_old[s_old] = (step, k)
                if s_new >= 0:
                    ring_new[s_new] = (step, k)
            written, wm1 = w2, wm2
            assert (wm1 + 1) & M32 == written and ring_old == ring_new
        assert written > 4 * 64                                  # several times round


def due_old(written, flushed):
    return (written >> 5) != flushed


def due_new(wm1, flushed):
    """flush_pipelined<true>: wm1 >= 32 flushed + 31 as SIGNED 32-bit values"""
    s = lambda v: v - (1 << 32) if v & 0x80000000 else v
    return s(wm1) >= s(((flushed << 5) + 31) & M32)


def test_flush_test_is_the_same_test():
    """Wherever a flush can stand - a half is read out as soon as it is complete, so `flushed` is written >> 5 or one
    less - the two conditions agree; in particular at a stream's start (wm1 = -1) and on both sides of every multiple
    of 32."""
    for written in list(range(0, 200)) + [32 * h + d for h in (1000, 16383, 2 ** 19, 2 ** 25) for d in (-2, -1, 0, 1, 2, 31)]:
        for flushed in {written >> 5, max((written >> 5) - 1, 0)}:
            assert due_new((written - 1) & M32, flushed) == due_old(written, flushed), (written, flushed)
    assert not due_new(M32, 0) and not due_new(30, 0) and due_new(31, 0) and not due_new(62, 1) and due_new(63, 1)


RING = 0x3e00                            # LDS address of a ring (16-byte aligned, not 64-byte aligned in general)
SEND = 0x7f0012345678                    # a stream's scratch end in global memory


def flush_old(written, flushed, k, ring=RING):
    """the parent's flush_pipelined on `written` / `flushed`: (due, LDS address read, global address of the half, flushed)"""
    due = due_old(written, flushed)
    return due, ring + (0 if flushed & 1 else 64) + 16 * k, SEND - 64 * (flushed + 1) + 16 * k, flushed + (1 if due else 0)


class FlushNew:
    """flush_pipelined<true>'s state between trip_enter and trip_leave: fthr = 32 flushed + 31, the LDS address of the
    half to read next (it changes sides through fsum - fhalf), and fdst = send + 16 k - 2, from which the half's place
    in the stream is fdst - 2 fthr."""

    def __init__(self, flushed, k, ring=RING):                   # trip_enter
        rk = ring + 16 * k
        self.fthr = ((flushed << 5) + 31) & M32
        self.fhalf = rk + (0 if flushed & 1 else 64)
        self.fsum = (2 * rk + 64) & M32
        self.fdst = SEND + 16 * k - 2

    def flush(self, wm1):
        s = lambda v: v - (1 << 32) if v & 0x80000000 else v
        due = s(wm1) >= s(self.fthr)
        read, dst = self.fhalf, self.fdst - ((2 * self.fthr) & M32)
        if due:
            self.fhalf = (self.fsum - self.fhalf) & M32
            self.fthr = (self.fthr + 32) & M32
        return due, read, dst

    def flushed(self):                                           # trip_leave
        return ((self.fthr - 31) & M32) >> 5


@pytest.mark.parametrize("q0", QUADS)
def test_loop_with_conversions_at_its_edges(q0):
    """The pipelined loop as the kernel runs it: trip_enter (wm1 = written - 1, fthr = 32 flushed + 31), double trips of
    eight steps with the flush in front of each, trip_leave (written = wm1 + 1, flushed = (fthr - 31) >> 5) - beside the
    parent's loop on `written` and `flushed`.  The flush fires in front of the same double trips (`written >> 5` changes
    exactly where it did), it reads the same half of the ring every time, due or not, a due half goes to the same place
    in the stream, and `flushed` and `written` come out alike - for a loop entered with words already written (the tail
    steps of phase A; 31 and 32: either side of a half), for every ring alignment mod 64, and for one that emits nothing."""
    rng = np.random.default_rng(11 + q0)
    for (start, rate), ring in zip(((0, 16), (3, 16), (0, 1), (2, 6), (31, 16), (32, 16), (0, 0)),
                                   (RING, RING + 16, RING + 32, RING + 48, RING + 80, RING, RING + 16)):
        for k in range(4):
            written, flushed = start, 0
            wm1, new = (written - 1) & M32, FlushNew(0, k, ring)          # trip_enter
            fired = []
            for d in range(60):
                due, read, dst, flushed = flush_old(written, flushed, k, ring)
                due_n, read_n, dst_n = new.flush(wm1)
                assert due_n == due and read_n == read, (start, rate, k, d)
                if due:
                    fired.append(d)
                    assert dst_n == dst, (start, rate, k, d)
                for _ in range(8):
                    pat = int(rng.integers(0, 16)) if rate == 16 else sum(1 << j for j in range(4) if rng.integers(0, 16) < rate)
                    m = pat << q0 | (int(rng.integers(0, 2 ** 63)) * 2 & ~(0xf << q0))
                    written = old_step(m, q0, written)[2]
                    wm1 = new_step(m, q0 + 3, wm1)[2]
                # a double trip of word steps completes at most one half: the flush never falls behind by two
                assert (written >> 5) - flushed <= 1
            assert new.flushed() == flushed and (wm1 + 1) & M32 == written      # trip_leave
            assert (len(fired) > 0) == (rate > 0)


def test_flush_state_from_any_flushed():
    """trip_enter with halves already flushed (odd and even, small and large): the carried form reads the half and names
    the place the parent's expressions do, before and after one due flush."""
    for flushed in (0, 1, 2, 3, 1000, 1001, 2 ** 19 + 1):
        for k in range(4):
            new = FlushNew(flushed, k)
            for step in range(3):
                written = 32 * (flushed + 1) + step                          # a half is due
                due, read, dst, f2 = flush_old(written, flushed, k)
                assert (due, read, dst) == new.flush((written - 1) & M32) and due
                flushed = f2
                assert new.flushed() == flushed
