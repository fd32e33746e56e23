// r4x16_enc_chain.h - k_enc_chain, the encoder's hot loop (rANS_static4x16pr.c:442-485, :794-839): device code shared by
// r4x16_enc_chain.hip (u16 images, order 0 and 1; the launcher) and r4x16_enc_chain_pk.hip (the packed-row
// instantiation, compiled with another instruction scheduler).
#pragma once
#include <stdlib.h>
#include <type_traits>
#include "r4x16_dev.h"
#include "r4x16_sched.h"
#include "r4x16_enc_step.h"

// General form: image in global memory, byte loads.  Used for the small nested streams inside
// k_enc_front and for alphabets whose tables do not fit LDS.
template <int ORDER>
__device__ __forceinline__ u32 chain_encode(gcu8 *data, u32 n, gcu8 *image, u32 ns, u32 bits, gcu32 *rcptab,
                                            gu8 *scratch_end, bool active, u32 lane)
{
    const u32 k = lane & 3;
    GAS const u16 *cum = (GAS const u16 *)(image + ENC_IMG_IDX);
    const u32 rs = ns + 1;
    u32 x = RANS_LOW;
    u32 written = 0;                 // words emitted by the quad so far
    u32 nsteps, first;               // this lane takes part in steps [first, nsteps)
    u32 p;                           // position of the symbol coded at this lane's next step
    const u32 q = n >> 2;
    if (ORDER == 0) {
        const u32 gtop = n ? (n - 1) >> 2 : 0;
        nsteps = n ? gtop + 1 : 0;
        first = (4 * gtop + k < n) ? 0 : 1;      // the top group may be partial (:442-448)
        p = 4 * (gtop - (first ? 1 : 0)) + k;    // unused when nsteps <= first
    } else {
        const u32 tail = n - 4 * q;              // extra bytes on chain 3 (:806-811)
        nsteps = tail + q;
        first = (k == 3) ? 0 : tail;
        p = (k == 3) ? n - 1 : k * q + q - 1;
    }
    if (!active) { nsteps = 0; first = 0; }

    u32 cur = 0;                                 // compact index of the symbol coded next
    if (nsteps > first) cur = image[data[p]];

    for (u32 s = 0; wave_any(s < nsteps); s++) {
        const bool live = s >= first && s < nsteps;
        bool emit = false;
        u32 rcp = 0, pk = 0, nextc = 0;
        if (live) {
            u32 row = 0;
            if (ORDER == 0) {
                if (p >= 4) nextc = image[data[p - 4]];
            } else if (s != nsteps - 1) {        // context = previous byte; quarter start: context 0
                nextc = image[data[p - 1]];
                row = nextc;
            }
            const u32 c0 = cum[row * rs + cur], c1 = cum[row * rs + cur + 1];
            pk = c0 | ((c1 - c0) << 16);
            rcp = enc_rcp(rcptab, c1 - c0);
            emit = enc_wants_emit(x, pk, bits);
        }
        const u32 em = quad_ballot(emit, lane);
        if (emit) {
            const u32 above = __popc(em >> (k + 1));
            *(gu16 *)(scratch_end - 2 * (written + above + 1)) = (u16)x;
            x >>= 16;
        }
        written += __popc(em);
        if (live) {
            x = enc_advance(x, rcp, pk, bits);
            cur = nextc;
            p -= (ORDER == 0) ? 4 : 1;
        }
    }
    // RansEncFlush x4 in order 3,2,1,0 (:482-485): R0 ends up lowest in memory
    if (active) *(gu32 *)(scratch_end - 2 * written - 16 + 4 * k) = x;
    return active ? 2 * written + 16 : 0;
}

// ---------------------------------------------------------------------------------------------
// Hot form, order-1: the image sits in LDS and nothing on the dependent path (the state x)
// touches memory.  Symbols are known in advance, so their table entries are fetched one trip
// (four steps) ahead: a trip issues the global load of the input dword two trips ahead, the LDS
// index lookups of the next trip's bytes and their entry reads, and then runs four state updates
// on entries that were loaded during the previous trip.
// The schedule is phased per wave: (A) up to three tail steps, chain 3 only; (B) whole trips of
// the backward walk; (B') its last 0..3 steps; (C) the quarter starts in context 0.  Streams of
// different lengths in one wave simply drop out of (B) at different trips.
// ---------------------------------------------------------------------------------------------
// Emitted 16-bit words are staged in a 128-byte LDS ring per stream and copied out 64 bytes at a
// time (16 bytes per lane).  Word j of a stream (emission order) belongs at scratch_end - 2 (j + 1);
// in the ring it sits at byte 126 - 2 (j & 63), which keeps each 64-byte half in memory order.
//
// Why: the wave's vector-memory counter retires in order, so ONE outstanding HBM access (an
// input prefetch, a store waiting for its acknowledgement) stalls every later wait on that
// counter.  The hot loop therefore keeps everything it consumes per trip in LDS (tables, the
// reciprocal table, the emitted words) and touches global memory exactly twice per eight steps,
// unconditionally and in a fixed order: one 8-byte input load three double-trips ahead and one
// 16-byte store (a completed half of the ring, or a dump slot nobody reads).
// (ENC_RING_BYTES, r4x16_common.h: the ring + a 2-byte dump slot for lanes that do not emit, padded)
#define ENC_LRCP_BYTES 16400u        // RCPTAB_ENTRIES dwords, padded to 16
// the frequency table of the packed rows' short-index kind (k_enc_chain<true, true, true>)
#define ENC_LFREQ_BYTES   8208u      // ENC_FREQTAB_ENTRIES 8-byte entries, padded to 16
static_assert(ENC_LFREQ_BYTES >= 8u * ENC_FREQTAB_ENTRIES && ENC_LFREQ_BYTES % 16u == 0, "frequency table in LDS");
// BYTE: rANS 4x8's renormalisation (rANS_byte.h:320-402: L = 2^23, up to TWO bytes per chain and step, 12-bit
// frequencies) on the same pipeline, ring and flush - round 4; the unit of `written` / the ring is then the byte.
template <bool BYTE>
struct EncOutT {
    u8 *ring;            // LDS
    u32 ring126;         // LDS address of the ring's last slot (word 126 / byte 127)
    gu8 *send;           // scratch_end of the stream
    gu8 *dump;           // this lane's 16 bytes of the dump area
    u32 written;         // words (bytes) emitted by the quad so far
    u32 flushed;         // 64-byte halves already read out of the ring
    u32 k, lane;
    bool active;
    u32x4 held;          // a half read out of the ring, stored one double-trip later
    gu8 *held_dst;
    u32 above = (0xeu << k) & 0xfu;                      // the quad's lanes that write before this one (chains k + 1 .. 3)
    u32 wm1 = 0, mlo = 0, mhi = 0;                       // trip_freq's form of `written` and its lane masks (trip_enter)
    u32 fthr = 0, fhalf = 0, fsum = 0;                   // flush_pipelined<true>'s form of `flushed` (trip_enter)
    gu8 *fdst = nullptr;
    static constexpr u32 HALF_SHIFT = BYTE ? 6u : 5u;    // units per 64-byte half, as a shift
    // the 16-bit renormalisation of one step (rANS_word.h:300-306): the state's low word into the ring where x is over
    // x_max; returns the state the step carries on with
    __device__ __forceinline__ u32 emit16(u32 x, bool live, bool over)
    {
        // the compare's own lane mask, and-ed with the live lanes on the scalar side (a ballot of the
        // combined predicate would be rebuilt through a select and a second compare)
        const u64 m = __ballot(over) & __ballot(live);
        const u32 em = (u32)(m >> (lane & ~3u)) & 0xfu;
        const bool emit = live && over;
        const u32 j = written + __popc(em >> (k + 1));
        const u32 j63 = emit ? (j & 63u) : ~0u;                          // -1: the dump slot at ring + 128
        *(LAS u16 *)(unsigned long)(ring126 - 2u * j63) = (u16)x;
        written += __popc(em);
        return emit ? x >> 16 : x;
    }
    // emit16 for the packed rows.  The same words at the same places, in fewer instructions: the lanes above this one are
    // counted through a per-lane mask and straight onto `written` (one and + one bit count with accumulate, no second shift
    // and no add), and the ring address is one multiply-add of the slot (-1: the dump slot, as above).
    // ALL: every lane's step is real or codes a neutral symbol (chain_encode_o1_lds), so there is no `live` to and in -
    // a neutral symbol has x_max = 2^31 and never emits.
    template <bool ALL>
    __device__ __forceinline__ u32 emit16q(u32 x, bool live, bool over)
    {
        const u64 m = ALL ? __ballot(over) : __ballot(over) & __ballot(live);
        const u32 em = (u32)(m >> (lane & ~3u));
        const bool emit = ALL ? over : live && over;
        const u32 j = written + __popc(em & above);
        const u32 j63 = emit ? (j & 63u) : ~0u;
        u32 a;
        asm("v_mad_i32_i24 %0, %1, -2, %2" : "=v"(a) : "v"(j63), "v"(ring126));   // (as shift + subtract otherwise)
        *(LAS u16 *)(unsigned long)a = (u16)x;
        written += __popc(em & 0xfu);
        return emit ? x >> 16 : x;
    }
    // rANS_word.h:281-321 for one symbol; x is this lane's state.  pk = start | freq << 16.
    // q = x / freq < 2^21 once x < x_max, so q * (M - freq) is a 24-bit multiply (mod 2^32).
    // Q: the packed rows' emit16q; ALL: no idle lanes (emit16q)
    template <bool Q = false, bool ALL = false>
    __device__ __forceinline__ void step(u32 &x, bool live, u32 rcp, u32 pk, u32 bits)
    {
        const u32 f = pk >> 16, start = pk & 0xffffu;
        u32 xs;
        if (BYTE) {
            // x_max = ((2^23 >> 12) << 8) * f; one byte while x >= x_max, a second one if x >> 8 still is
            const u32 x_max = f << 19;
            const bool o1 = x >= x_max, o2 = (x >> 8) >= x_max;
            const u64 lv = __ballot(live);
            const u32 e1 = (u32)((__ballot(o1) & lv) >> (lane & ~3u)) & 0xfu, e2 = (u32)((__ballot(o2) & lv) >> (lane & ~3u)) & 0xfu;
            const bool emit1 = live && o1, emit2 = live && o2;
            const u32 j = written + __popc(e1 >> (k + 1)) + __popc(e2 >> (k + 1));
            const u32 j1 = emit1 ? (j & 127u) : ~0u, j2 = emit2 ? ((j + 1u) & 127u) : ~0u;       // -1: the dump slot at ring + 128
            *(LAS u8 *)(unsigned long)(ring126 - j1) = (u8)x;
            *(LAS u8 *)(unsigned long)(ring126 - j2) = (u8)(x >> 8);
            xs = emit2 ? x >> 16 : emit1 ? x >> 8 : x;
            written += __popc(e1) + __popc(e2);
        } else xs = Q ? emit16q<ALL>(x, live, x >= (f << (31u - bits))) : emit16(x, live, x >= (f << (31u - bits)));
        // exact x / f: Alverson reciprocal for f >= 2; f == 1 has rcp = 2^32 - 1 and shift 0, which
        // gives x - 1: the compare's carry puts the 1 back (an add-with-carry, no select)
        const u32 fm1 = f - 1u;
        const u32 rsh = 31u - (u32)__clz((int)(fm1 | 1u));
        const u32 q = (__umulhi(xs, rcp) >> rsh) + (fm1 == 0u ? 1u : 0u);
        const u32 cmpl = (1u << bits) - f;
        const u32 xn = __umul24(q, cmpl) + (xs + start);
        x = ALL || live ? xn : xs;
    }
    // The step of the short-index packed rows (10-bit tables): {m, w} is the frequency table's entry of f (r4x16_api.hip),
    // w = (1024 - f) | s << 24, and nothing is derived from f here, not even x_max.  The same x as step(), bit for bit:
    // both compute xs + start + (xs / f) * (1024 - f) with the exact quotient of a state xs < 2^31.
    //   q: m is the low word of the round-up reciprocal ceil(2^(32 + s) / f), s = ceil(log2 f), which lies in
    //      [2^32, 2^33): (mulhi(xs, m) + xs) >> s = floor(xs * (2^32 + m) / 2^(32 + s)) = xs / f for every 32-bit xs; the
    //      sum stays below 2^32 because mulhi(xs, m) < xs < 2^31.  step() has the reciprocal of shift s - 1, exact below 2^31.
    //      f = 1: s = 0, m = 0, q = xs - what step() reaches with reciprocal 2^32 - 1, xs - 1 and the compare's carry.
    //      f = 2 (any power of two): m = 0, q = xs >> s.      f = 3 (no power of two): m = ceil(2^(32 + s) / f) - 2^32 > 0.
    //   q * (1024 - f): q < 2^21 and 1024 - f < 2^10, a 24-bit multiply that does not look at the shift in w's top byte
    //      (the symbol records' trick, r4x16_common.h).  f = 1024: w's low bits are 0, the product is 0 and x = xs + start.
    // X is x_max = f << 21 as it comes out of the row (chain_encode_o1_lds' topk): the compare takes it as it is.
    template <bool ALL = false>
    __device__ __forceinline__ void step_freq(u32 &x, bool live, u32 m, u32 w, u32 start, u32 X)
    {
        const u32 xs = emit16q<ALL>(x, live, x >= X);
        const u32 q = (__umulhi(xs, m) + xs) >> ((w >> 24) & 31u);
        const u32 xn = __umul24(q, w) + (xs + start);
        x = ALL || live ? xn : xs;
    }
    // step_freq<true> for the four steps of a trip of the pipelined loop, written out as ONE statement because the order
    // is the change.  The same x and the same words at the same places:
    //  - `emit ? x >> 16 : x` is ONE select with a word pick (SDWA), which takes its condition from vcc only - the C++ form
    //    has the compare as a bool beside a ballot and gets a shift and a select;
    //  - a vector instruction reads vcc two slots behind the compare that wrote it at the earliest.  Nothing of the step
    //    itself can stand there (all of it hangs on the compare), so the PREVIOUS step's ring write and DPP move do
    //    (ENC_TRIP_WRITE); the first step has the starts of two of the next trip's symbols there, and the last step's
    //    write and move stand at the end;
    //  - a lone wave issues an instruction that reads its predecessor's result 1.7 slots behind it (profiles/enc_quad.md),
    //    so the count's instructions alternate with the division's and the ring address closes the step: every
    //    instruction stands at least two slots behind the one it reads from;
    //  - one statement, not one per step: the compiler puts an idle slot between a statement and the next instruction
    //    or statement that reads one of its outputs, and every piece of a step reads the one before.
    // The state alternates between two registers (xa, xb), so the one a step started from is still there when the next
    // step writes its low word out.
    // The quad's count (trip_enter): a quad lies wholly in lanes 0..31 or wholly in lanes 32..63, so the compare's mask is
    // and-ed half by half with two lane constants of which one is 0 - `mlo` / `mhi` hold, at the quad's place in its half,
    // this lane's bit and those of the quad's lanes that write before it (chains k .. 3).  Each instruction reads one
    // scalar register, which is what VOP2 / VOP3 allow.  One bit count with accumulate onto `wm1` - the words written by
    // the quad so far, MINUS ONE - gives t = wm1 + (emitting lanes among this one and those before it): an emitting
    // lane's own slot, where `written` + (those before it) stood.  The quad's lane 0 counts the whole quad, so its t is
    // the next step's wm1: one DPP move (quad_perm 0,0,0,0) brings it to the four lanes.  No 64-bit shift, no second
    // mask, no second count, no fixed register pair.  (tests/test_enc_quad_cpu.py: the count against emit16q's.)
    // The ring writes are not counted by the compiler's LDS waits, which is safe: LDS operations return in order and a
    // wait for "at most N outstanding" can only cover more with an operation it does not know of.
    // Hazards inside (gfx950): vcc written by a compare is read 3 slots later at the earliest; a DPP operand is read two
    // slots behind the vector instruction that wrote it at the earliest - the move stands in the NEXT step's compare
    // slots, eight instructions behind the count; the SDWA forms write whole dwords (no forwarding hazard); nothing
    // else here is on the list.
    // Every lane of the wave runs the statement (lanes without a stream code neutral symbols), so the move's source lane
    // is always enabled.
#define ENC_TRIP_WRITE(xp) \
        "ds_write_b16 %[pj], %[" xp "]\n\t" \
        "v_mov_b32_dpp %[wm1], %[t] quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\t"
#define ENC_TRIP_STEP(gap, xi, xo, n) \
        "v_cmp_ge_u32_e32 vcc, %[" xi "], %[X" n "]\n\t" \
        gap \
        "v_cndmask_b32_sdwa %[xs], %[" xi "], %[" xi "], vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1\n\t" \
        "v_and_b32_e32 %[t], vcc_lo, %[mlo]\n\t" \
        "v_mul_hi_u32 %[q], %[xs], %[m" n "]\n\t" \
        "v_and_or_b32 %[t], vcc_hi, %[mhi], %[t]\n\t" \
        "v_add_u32_e32 %[q], %[xs], %[q]\n\t" \
        "v_bcnt_u32_b32 %[t], %[t], %[wm1]\n\t" \
        "v_lshrrev_b32_sdwa %[q], %[w" n "], %[q] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD\n\t" \
        "v_and_b32_e32 %[pj], 63, %[t]\n\t" \
        "v_mul_u32_u24_e32 %[q], %[q], %[w" n "]\n\t" \
        "v_cndmask_b32_e32 %[pj], -1, %[pj], vcc\n\t" \
        "v_add3_u32 %[" xo "], %[xs], %[s" n "], %[q]\n\t" \
        "v_mad_i32_i24 %[pj], %[pj], -2, %[r126]\n\t"
    // the lane constants of the statement's count, and `written` -> wm1: once, in front of the pipelined loop
    __device__ __forceinline__ void trip_enter()
    {
        const u32 aos = (above | 1u << k) << (lane & 28u);
        mlo = lane < 32u ? aos : 0u;
        mhi = lane < 32u ? 0u : aos;
        wm1 = written - 1u;
        fthr = (flushed << 5) + 31u;
        const u32 rk = (u32)(unsigned long)(LAS u8 *)ring + 16u * k;
        fhalf = rk + ((flushed & 1u) ? 0u : 64u);
        fsum = 2u * rk + 64u;
        fdst = send + 16u * k - 2;
    }
    // wm1 -> `written`, fthr -> `flushed`: once, behind the loop; everything outside it reads those
    __device__ __forceinline__ void trip_leave() { written = wm1 + 1u; flushed = (fthr - 31u) >> 5; }
    // na, nb: two pairs of the NEXT trip as they come out of the row; their starts (the low eleven bits) are taken in the
    // two slots behind the first compare, where the first step has no ring write to place.
    __device__ __forceinline__ void trip_freq(u32 &x, u32x4 m, u32x4 w, u32 s0, u32 s1, u32 s2, u32 s3, u32 X0, u32 X1, u32 X2, u32 X3,
                                              u32 &na, u32 &nb)
    {
        u32 xb, xs, t, q, pj;
        asm volatile(ENC_TRIP_STEP("v_and_b32_e32 %[na], 0x7ff, %[na]\n\t"
                                   "v_and_b32_e32 %[nb], 0x7ff, %[nb]\n\t", "xa", "xb", "0")
                     ENC_TRIP_STEP(ENC_TRIP_WRITE("xa"), "xb", "xa", "1")
                     ENC_TRIP_STEP(ENC_TRIP_WRITE("xb"), "xa", "xb", "2")
                     ENC_TRIP_STEP(ENC_TRIP_WRITE("xa"), "xb", "xa", "3")
                     ENC_TRIP_WRITE("xb")
                     : [xa] "+v"(x), [wm1] "+v"(wm1), [na] "+v"(na), [nb] "+v"(nb), [xb] "=&v"(xb), [xs] "=&v"(xs), [t] "=&v"(t), [q] "=&v"(q), [pj] "=&v"(pj)
                     : [mlo] "v"(mlo), [mhi] "v"(mhi), [r126] "v"(ring126),
                       [m0] "v"(m.x), [w0] "v"(w.x), [s0] "v"(s0), [X0] "v"(X0), [m1] "v"(m.y), [w1] "v"(w.y), [s1] "v"(s1), [X1] "v"(X1),
                       [m2] "v"(m.z), [w2] "v"(w.z), [s2] "v"(s2), [X2] "v"(X2), [m3] "v"(m.w), [w3] "v"(w.w), [s3] "v"(s3), [X3] "v"(X3)
                     : "vcc", "memory");
    }
    // conditional form: copy out the half that has just been completed, if any
    __device__ __forceinline__ void flush()
    {
        const bool due = active && (written >> HALF_SHIFT) != flushed;
        if (wave_any(due)) {
            if (due) {
                const u32x4 v = *(const u32x4 *)(ring + ((flushed & 1u) ? 0u : 64u) + 16u * k);
                *(GAS u32x4_unaligned *)(send - 64ull * (flushed + 1u) + 16u * k) = v;
                flushed++;
            }
        }
    }
    // unconditional form for the main loop: store what was read out last time, read out the next
    // WM1: between trip_enter and trip_leave, where wm1 = written - 1 is what the steps carry and `flushed` is carried as
    // fthr = 32 flushed + 31.  written >> 5 != flushed means written >= 32 (flushed + 1), as a half is read out as soon
    // as it is complete: wm1 >= fthr, signed (wm1 starts at -1).  The half to read next is an LDS address that changes
    // sides when a half is due (fhalf, fsum - fhalf), and the place of the half in the stream is send - 64 (flushed + 1)
    // + 16 k = (send + 16 k - 2) - 2 fthr: a shift and a 64-bit subtract, no multiply under a branch.
    template <bool WM1 = false>
    __device__ __forceinline__ void flush_pipelined()
    {
        *(GAS u32x4_unaligned *)held_dst = held;
        if (WM1) {
            const bool due = active && (int)wm1 >= (int)fthr;
            held = *(LAS const u32x4 *)(unsigned long)fhalf;
            gu8 *dst = fdst - (u64)(2u * fthr);
            held_dst = due ? dst : dump;
            fhalf = due ? fsum - fhalf : fhalf;
            fthr += due ? 32u : 0u;
            return;
        }
        const bool due = active && (written >> HALF_SHIFT) != flushed;
        held = *(const u32x4 *)(ring + ((flushed & 1u) ? 0u : 64u) + 16u * k);
        held_dst = due ? send - 64ull * (flushed + 1u) + 16u * k : dump;
        flushed += due ? 1u : 0u;
    }
    __device__ __forceinline__ void flush_drain()
    {
        *(GAS u32x4_unaligned *)held_dst = held;
        held_dst = dump;
    }
    // the words (bytes) still in the ring, then the four states (RansEncFlush in order 3,2,1,0, :482-485)
    __device__ __forceinline__ u32 finish(u32 x)
    {
        flush();
        if (BYTE) { flush(); }                           // (a double trip of byte steps can complete two halves)
        const u32 first = (BYTE ? 64u : 32u) * flushed;
        const u32 rem = active ? written - first : 0u;
        for (u32 i = k; wave_any(i < rem); i += 4) {
            if (i < rem) {
                const u32 j = first + i;
                if (BYTE) send[-(long)(j + 1u)] = *(const u8 *)(ring + (127u - (j & 127u)));
                else *(gu16 *)(send - 2ull * (j + 1u)) = *(const u16 *)(ring + ((~j << 1) & 126u));
            }
        }
        if (active) {
            if (BYTE) { gu8 *d = send - written - 16 + 4 * k; d[0] = (u8)x; d[1] = (u8)(x >> 8); d[2] = (u8)(x >> 16); d[3] = (u8)(x >> 24); }
            else *(gu32 *)(send - 2ull * written - 16 + 4 * k) = x;
        }
        return active ? (BYTE ? written : 2 * written) + 16 : 0;
    }
};
typedef EncOutT<false> EncOut;

// PK: packed rows (r4x16_common.h) and a reciprocal table of the 1,025 frequencies a 10-bit table can hold.
// FT: the packed rows' short-index kind: idx_of[0..127] only, and `lrcp` is the frequency table (8-byte entries, read whole
// where the reciprocal alone was read; EncOutT::step_freq).
// aff_wave (FT only, the same in every lane): every stream of the wave has an affine alphabet, compact index = byte - c
// (EncItem.affine = c + 1, `aff`): the pipelined loop computes its index words from the bytes, with no idx_of[] look-up.
template <bool PK, bool BYTE = false, bool FT = false>
__device__ __forceinline__ u32 chain_encode_o1_lds(const u8 *img_lds, u8 *ring, const u32 *lrcp, gcu8 *data, u32 n, u32 ns,
                                                   u32 bits, gcu8 *safe, gu8 *scratch_end, gu8 *dump, bool active, u32 lane,
                                                   bool aff_wave = false, u32 aff = 0u)
{
    const u32 k = lane & 3;
    static_assert(!FT || (PK && !BYTE), "the frequency table serves the packed rows");
    if (PK) bits = 10u;              // what packed rows are made for - and what a lane WITHOUT a stream must code its neutral symbols with
    const u8 *idx = img_lds;
    const u8 *cumb = img_lds + (FT ? ENC_IMG_IDX_SHORT : ENC_IMG_IDX);
    const u32 rs = PK ? 4u * enc_pk_row_dwords(ns) : ns + 1;       // bytes (packed) / u16 entries per context row
    const u32 cumb_lds = (u32)(unsigned long)(LAS const u8 *)cumb;
    // the (start, next) pair of symbol si in context ci.  u16 rows: start | next << 16, one dword read at a 2-byte
    // aligned LDS address.  Packed rows: 22 bits at bit 11 si of the row, from two aligned dwords and a funnel shift.
    // Packed rows: everything a look-up takes from a compact index j comes out of ONE multiply-add, the index's word
    //     11 j  |  (dword address of row j) << 16         (11 j <= 693; an LDS dword address is below 2^16)
    // - an index is the symbol of one step and the context of the next (cum4), so it used to be multiplied twice.  The pair of
    // symbol si in context ci starts at dword word(ci) >> 16 + (11 si >> 5), bit 11 si & 31.  u16 rows: the word is the index.
    const u32 wmul = PK ? 11u | (rs >> 2) << 16 : 1u, wadd = PK ? (cumb_lds >> 2) << 16 : 0u;
    auto word = [&](u32 j) -> u32 {
        if (!PK) return j;
        u32 w = __umul24(j, wmul) + wadd;
        asm("" : "+v"(w));               // one word: without this the low half is multiplied a second time, without the add
        return w;
    };
    auto pairr = [&](u32 wc, u32 ws) -> u32x2 {          // packed rows: the two dwords that hold the pair
        const u32 a = ((wc >> 16) + __builtin_amdgcn_ubfe(ws, 5, 5)) << 2;
        return *(LAS const u32x2_a4 *)(unsigned long)a;
    };
    auto pairw = [&](u32 wc, u32 ws) -> u32 {
        if (PK) {
            const u32x2 d = pairr(wc, ws);
            return __builtin_amdgcn_alignbit(d.y, d.x, ws);                  // (the shift uses the low five bits of ws)
        }
        return *(LAS const u32 *)(cumb + 2u * (__umul24(wc, rs) + ws));
    };
    auto pair = [&](u32 ci, u32 si) -> u32 { return pairw(word(ci), word(si)); };
    // Packed rows: the pair of a NEUTRAL symbol, {start 0, next 1 << bits} (their tables have 10 bits): frequency 1,024 has
    // x_max = 2^31, which no state reaches, and 1024 - f = 0, so a step that codes it leaves x and the ring as they are.
    // The pipelined loop hands it to every lane that has no symbol to code in a trip, and therefore
    //  - its steps need no `live` (EncOutT::emit16q<ALL>), and
    //  - every pair that reaches rcpof() is this one or a pair of the stream's own bytes in the stream's own rows, whose
    //    entries ascend from 0 to 1,024: 0 <= f <= 1,024 and the table index stays inside the table with no clamp.  The
    //    other phases fetch() for live lanes only.
    const u32 neutral = 1024u << 11;
    const u32 rcp_last = RCPTAB_ENTRIES - 1u;
    // A symbol on its way to its step: pk = start | freq << 16; FT: pk = start and f = x_max = freq << 21, which is all the
    // step and the table read want of the frequency (topk below)
    // (every instruction of the loop is issue time, on the dependent path or off it: no packing that a step undoes again)
    struct PF { u32 pk, f; };
    // {reciprocal, 0}, or the frequency table's entry  (u16 rows clamp: their idle lanes hold garbage; packed rows: above)
    // FT: entry f is 8 bytes at LDS byte address 8 f = x_max >> 18, one shift - the frequency table stands at LDS address
    // 0: k_enc_chain puts it at the start of its dynamic LDS and has no static LDS in front of it (the flag of "does
    // anybody have work" lives in the dynamic LDS for that reason; the parent's listing formed this address with a
    // literal 0 already).  A table anywhere else needs its address added here - one instruction per symbol.
    auto rcpof = [&](PF s) -> u32x2 {
        if (FT) return *(LAS const u32x2 *)(unsigned long)(s.f >> 18);
        const u32 f = s.pk >> 16;
        u32x2 r = {lrcp[PK ? f : f < rcp_last ? f : rcp_last], 0u};
        return r;
    };
    // pair -> start | freq << 16.  u16 rows: a shift and a subtract (the empty asm keeps it from becoming a
    // quarter-rate multiply by 0xFFFF0001); packed rows: two field extractions, a subtract, a shift-or.
    // FT: start, and x_max = (next - start) << 21 by ONE multiply.  p is what v_alignbit delivers: start in bits 0..10, next
    // in bits 11..21, the row's following fields above.  p * (2^10 - 2^21) = start * 2^10 + (next - start) * 2^21 mod 2^32:
    // p * 2^10 carries next to bit 21, p * 2^21 carries start there, and whatever p holds above bit 21 - the sign bit of
    // the 24-bit operand included - lands on multiples of 2^32.  start * 2^10 < 2^21 stays below the field and is masked
    // off.  The neutral pair gives 2^31.  (tests/test_enc_xmax_cpu.py: every pair, any upper bits.)  Written as asm: the
    // multiplier is hidden from the compiler, which makes two shifts and a subtract of a constant one.
    int xmul = 1024 - 2097152;
    if (FT) asm("" : "+s"(xmul));
    // late: the start stays unmasked, EncOutT::trip_freq takes it.
    auto topk = [&](u32 p, bool late = false) -> PF {
        if (FT) {
            const u32 X = (u32)__mul24((int)p, xmul);
            PF r = {late ? p : p & 2047u, X & 0xffe00000u};
            return r;
        }
        if (PK) {
            const u32 st = p & 2047u, f = __builtin_amdgcn_ubfe(p, 11, 11) - st;
            PF r = {st | (f << 16), f};
            return r;
        }
        u32 hi = p << 16; asm("" : "+v"(hi));
        PF r = {p - hi, 0u};
        return r;
    };
    struct Sym { u32 rcp, w; PF s; };                     // {reciprocal, second word of the frequency table, the symbol}
    auto fetch = [&](u32 ci, u32 si) -> Sym {
        const PF s = topk(pair(ci, si));
        const u32x2 e = rcpof(s);
        Sym r = {e.x, e.y, s};
        return r;
    };
    auto step = [&](EncOutT<BYTE> &o, u32 &x, bool live, u32 rcp, u32 w, u32 pk, u32 f) {
        if (FT) o.step_freq(x, live, rcp, w, pk, f);
        else o.template step<PK>(x, live, rcp, pk, bits);
    };
    auto step_all = [&](EncOutT<BYTE> &o, u32 &x, u32 rcp, u32 w, u32 pk, u32 f) {        // packed rows, pipelined loop
        if (FT) o.template step_freq<true>(x, true, rcp, w, pk, f);
        else o.template step<true, true>(x, true, rcp, pk, bits);
    };
    EncOutT<BYTE> o{ring, (u32)(unsigned long)(LAS u8 *)ring + (BYTE ? 127u : 126u), scratch_end, dump, 0u, 0u, k, lane, active, {0, 0, 0, 0}, dump};
    u32 x = BYTE ? (1u << 23) : RANS_LOW;
    const u32 q = active ? n >> 2 : 0;
    const u32 tail = active ? n - 4 * q : 0;

    // (A) tail bytes n-1 .. 4q on chain 3, context = previous byte (:806-811)
    u32 cur = 0;
    if (active && k == 3 && tail) cur = idx[data[n - 1]];
    for (u32 s = 0; wave_any(s < tail); s++) {
        const bool live = k == 3 && s < tail;
        Sym e = {0, 0, {0, 0}};
        if (live) {
            const u32 ci = idx[data[n - 2 - s]];
            e = fetch(ci, cur);
            cur = ci;
        }
        step(o, x, live, e.rcp, e.w, e.s.pk, e.s.f);
    }

    // (B) backward walk over offsets q-1 .. 1 of each quarter (:813-829); chain k codes byte
    // k*q + r in context byte k*q + r - 1.  Trip t codes offsets r0-4t .. r0-4t-3; the pipelined
    // loop takes an even number of trips, the rest goes to (B').
    gcu8 *qbase = data + (u64)k * q;
    const u32 r0 = q ? q - 1 : 0;
    const u32 main = r0;                         // steps in (B)+(B')
    const u32 npair = main >> 3;                 // double trips
    const u32 ntrip = 2 * npair;
    cur = (active && q) ? idx[qbase[r0]] : 0u;
    // AFF (the short-index kind, a wave whose streams all have affine alphabets): the loop's index words are computed from
    // the bytes - idx4 below.
    auto pipelined = [&](auto affc) {
        constexpr bool AFF = decltype(affc)::value;
        // Software pipeline, every access issued at least one trip before its first use:
        //   input piece of double-trip D+3 (HBM, 8 bytes)   byte -> compact index of trip t+3 (LDS)
        //   cumulative pair of trip t+2 (LDS)               reciprocal of trip t+1 (LDS)      trip t: 4 state updates
        // Pieces are asked for in order, j = 0, 1, 2 ..: a saturating offset walks down the quarter and stops at its
        // start, so a lane past its last double trip reads the quarter's first eight bytes again (npair > 0: the quarter
        // has nine or more) and a lane with no double trip at all reads `safe`.  Their trips code neutral symbols.
        gcu8 *lbase = npair ? qbase : safe;
        u32 loff = npair ? r0 : 0u;
        auto load8 = [&](u32 j) -> u32x2 {       // bytes r0-8j-8 .. r0-8j-1: .y = contexts of trip 2j, .x = of trip 2j+1
            if (!PK) {
                gcu8 *p = j < npair ? qbase + (r0 - 8 * j) - 8 : safe;
                return *(GAS const u32x2_unaligned *)p;
            }
            loff = __builtin_elementwise_sub_sat(loff, 8u);
            return *(GAS const u32x2_unaligned *)(lbase + loff);
        };
        struct I4 { u32 c0, c1, c2, c3; };       // the words of four compact indices
        // AFF: word(byte - c) = byte * wmul + (wadd - c * wmul) mod 2^32 - one multiply-add of the byte with two constants
        // of the lane, no idx_of[] read (both halves of the sum are in range, so what the addend borrows across bit 16
        // comes back; tests/test_enc_affine_cpu.py).  That holds for a lane's own data, whose bytes are members of its
        // alphabet - the pieces of its double trips, and its quarter's first bytes, which it reads again past its last one.
        // A lane without a double trip reads `safe` or nothing of its own: its word must not depend on the byte, so its
        // multiplier is 0 and its addend the word of index 0 in the image it holds - a valid pair address, whose pair
        // real4 replaces by the neutral one.
        u32 amul = 0u, aadd = wadd;
        if (AFF && npair) { amul = wmul; aadd = wadd - __umul24(aff - 1u, wmul); }
        auto aword = [&](u32 b) -> u32 {
            u32 w = __umul24(b, amul) + aadd;
            asm("" : "+v"(w));               // (one multiply-add, as in word())
            return w;
        };
        auto idx4 = [&](u32 ww) -> I4 {
            if (AFF) {
                I4 r = {aword(ww >> 24), aword((ww >> 16) & 0xff), aword((ww >> 8) & 0xff), aword(ww & 0xff)};
                return r;
            }
            I4 r = {word(idx[ww >> 24]), word(idx[(ww >> 16) & 0xff]), word(idx[(ww >> 8) & 0xff]), word(idx[ww & 0xff])};
            return r;
        };
        auto cum4 = [&](const I4 &c, u32 sym) -> u32x4 {     // raw pairs start | next << 16
            if (FT) {
                // the four funnel shifts as one statement: the compiler then waits ONCE for the four reads (they return
                // in order, and it gives each shift a counted wait of its own - three issue slots per trip).  Nothing
                // reads the pairs before the next trip, so no idle slot follows the statement.
                const u32x2 d0 = pairr(c.c0, sym), d1 = pairr(c.c1, c.c0), d2 = pairr(c.c2, c.c1), d3 = pairr(c.c3, c.c2);
                u32x4 r;
                asm("v_alignbit_b32 %0, %4, %5, %6\n\t"
                    "v_alignbit_b32 %1, %7, %8, %9\n\t"
                    "v_alignbit_b32 %2, %10, %11, %12\n\t"
                    "v_alignbit_b32 %3, %13, %14, %15"
                    : "=&v"(r.x), "=&v"(r.y), "=&v"(r.z), "=v"(r.w)
                    : "v"(d0.y), "v"(d0.x), "v"(sym), "v"(d1.y), "v"(d1.x), "v"(c.c0), "v"(d2.y), "v"(d2.x), "v"(c.c1),
                      "v"(d3.y), "v"(d3.x), "v"(c.c2));
                return r;
            }
            u32x4 r = {pairw(c.c0, sym), pairw(c.c1, c.c0), pairw(c.c2, c.c1), pairw(c.c3, c.c2)};
            return r;
        };
        auto real4 = [&](u32x4 p, bool live) -> u32x4 {      // packed rows: neutral symbols for a lane without a trip
            if (!PK) return p;
            u32x4 r = {live ? p.x : neutral, live ? p.y : neutral, live ? p.z : neutral, live ? p.w : neutral};
            return r;
        };
        struct P4 { PF x, y, z, w; };
        auto topk4 = [&](u32x4 p, bool late = false) -> P4 {     // late: the first two starts are left to the trip's statement
            P4 r = {topk(p.x, late), topk(p.y, late), topk(p.z), topk(p.w)};
            return r;
        };
        struct R4 { u32x4 rcp, w; };
        auto rcp4 = [&](const P4 &p) -> R4 {
            const u32x2 a = rcpof(p.x), b = rcpof(p.y), c = rcpof(p.z), d = rcpof(p.w);
            R4 r = {{a.x, b.x, c.x, d.x}, {a.y, b.y, c.y, d.y}};
            return r;
        };
        u32 cur1, cur2;
        I4 I2;
        P4 P0;
        u32x4 Praw;
        R4 R0;
        // input pieces live in a ring of four register pairs, piece j in Q[j % 4]; the loop is unrolled
        // four double-trips so that no piece is ever copied (a copy would have to wait for the load)
        u32x2 Q0, Q1, Q2, Q3;
        {
            Q0 = load8(0); Q1 = load8(1); Q2 = load8(2); Q3 = load8(3);
            const I4 i0 = idx4(Q0.y), i1 = idx4(Q0.x);
            I2 = idx4(Q1.y);
            P0 = topk4(real4(cum4(i0, word(cur)), 0 < ntrip));
            Praw = cum4(i1, i0.c3);
            cur1 = i0.c3; cur2 = i1.c3;
            R0 = rcp4(P0);
        }
        u32 t = 0;
        auto trip = [&](u32 wnext3) {
            const bool live = t < ntrip;
            const I4 In = idx4(wnext3);              // bytes of trip t+3
            const u32x4 Pn = cum4(I2, cur2);         // pairs of trip t+2
            P4 P1 = topk4(real4(Praw, t + 1 < ntrip), FT);       // trip t+1, read during the previous trip
            const R4 Rn = rcp4(P1);
            // the look-ups above belong to later trips: keep the scheduler from pulling next trip's
            // (which depend on them) up behind them, which would put their latency on this trip
            __builtin_amdgcn_sched_barrier(0);
            if (FT) {
                o.trip_freq(x, R0.rcp, R0.w, P0.x.pk, P0.y.pk, P0.z.pk, P0.w.pk, P0.x.f, P0.y.f, P0.z.f, P0.w.f, P1.x.pk, P1.y.pk);
            } else if (PK) {
                step_all(o, x, R0.rcp.x, R0.w.x, P0.x.pk, P0.x.f);
                step_all(o, x, R0.rcp.y, R0.w.y, P0.y.pk, P0.y.f);
                step_all(o, x, R0.rcp.z, R0.w.z, P0.z.pk, P0.z.f);
                step_all(o, x, R0.rcp.w, R0.w.w, P0.w.pk, P0.w.f);
            } else {
                step(o, x, live, R0.rcp.x, R0.w.x, P0.x.pk, P0.x.f);
                step(o, x, live, R0.rcp.y, R0.w.y, P0.y.pk, P0.y.f);
                step(o, x, live, R0.rcp.z, R0.w.z, P0.z.pk, P0.z.f);
                step(o, x, live, R0.rcp.w, R0.w.w, P0.w.pk, P0.w.f);
                if (live) cur = cur1;
            }
            cur1 = cur2; cur2 = I2.c3;
            I2 = In; P0 = P1; Praw = Pn; R0 = Rn;
            t++;
            __builtin_amdgcn_sched_barrier(0);
        };
        // double-trip d: trip 2d looks up the bytes of trip 2d+3 (piece d+1, low dword), trip 2d+1
        // those of trip 2d+4 (piece d+2, high dword); piece d+4 is requested into the slot of piece d
        if (FT) o.trip_enter();
        for (u32 d = 0; wave_any(d < npair); d += 4) {
            Q0 = load8(d + 4); o.template flush_pipelined<FT>(); trip(Q1.x); trip(Q2.y);
            Q1 = load8(d + 5); o.template flush_pipelined<FT>(); trip(Q2.x); trip(Q3.y);
            Q2 = load8(d + 6); o.template flush_pipelined<FT>(); trip(Q3.x); trip(Q0.y);
            Q3 = load8(d + 7); o.template flush_pipelined<FT>(); trip(Q0.x); trip(Q1.y);
        }
        if (FT) o.trip_leave();
        o.flush_drain();
        o.flush();                               // fewer than 32 words may stay in the ring from here on
        // (packed rows: the loop does not carry the symbol that follows its last live trip - it is read again)
        if (PK) cur = (active && q) ? idx[qbase[r0 - 4 * ntrip]] : 0u;
    };
    if (wave_any(npair > 0)) {
        if constexpr (FT) {
            if (aff_wave) pipelined(std::true_type{});
            else pipelined(std::false_type{});
        } else pipelined(std::false_type{});
    }
    // (B') remaining walk steps, one at a time
    u32 r = r0 - 4 * ntrip, done = 4 * ntrip;
    for (; wave_any(done < main); ) {
        const bool live = done < main;
        Sym e = {0, 0, {0, 0}};
        if (live) {
            const u32 ci = idx[qbase[r - 1]];
            e = fetch(ci, cur);
            cur = ci; r--; done++;
        }
        step(o, x, live, e.rcp, e.w, e.s.pk, e.s.f);
        o.flush();
    }
    // (C) first byte of each quarter in context 0 (:831-834)
    {
        const bool live = active && q > 0;
        Sym e = {0, 0, {0, 0}};
        if (live) e = fetch(0, cur);
        step(o, x, live, e.rcp, e.w, e.s.pk, e.s.f);
    }
    return o.finish(x);
}

// Hot form, order-0, for the chain kernel: the same software pipeline as chain_encode_o1_lds over
// the one-row image (:442-459: step s codes group g = gtop - s, chain k takes byte 4g + k; the top
// group may be partial).  A trip of four steps covers four whole groups = 16 contiguous bytes, of
// which this lane uses byte k of each dword.
template <bool BYTE = false>
__device__ __forceinline__ u32 chain_encode_o0_pipe(const u8 *img_lds, u8 *ring, const u32 *lrcp, gcu8 *data, u32 n,
                                                    u32 bits, gcu8 *safe, gu8 *scratch_end, gu8 *dump, bool active, u32 lane)
{
    const u32 k = lane & 3;
    const u8 *idx = img_lds;
    const u8 *cumb = img_lds + ENC_IMG_IDX;
    auto pair = [&](u32 si) -> u32 { return *(LAS const u32 *)(cumb + 2u * si); };
    auto rcpof = [&](u32 pk) -> u32 { const u32 f = pk >> 16; return lrcp[f < RCPTAB_ENTRIES - 1u ? f : RCPTAB_ENTRIES - 1u]; };
    auto topk = [&](u32 p) -> u32 { u32 hi = p << 16; asm("" : "+v"(hi)); return p - hi; };
    auto fetch = [&](u32 si) -> u32x2 {
        const u32 pk = topk(pair(si));
        u32x2 r = {rcpof(pk), pk};
        return r;
    };
    EncOutT<BYTE> o{ring, (u32)(unsigned long)(LAS u8 *)ring + (BYTE ? 127u : 126u), scratch_end, dump, 0u, 0u, k, lane, active, {0, 0, 0, 0}, dump};
    u32 x = BYTE ? (1u << 23) : RANS_LOW;
    const u32 Q = active ? n >> 2 : 0;                    // whole groups
    const u32 rem = active ? n & 3u : 0;                  // bytes of the partial top group

    // (A) the partial top group: chains k < rem code byte 4Q + k
    if (wave_any(rem != 0)) {
        const bool live = k < rem;
        u32 rcp = 0, pk = 0;
        if (live) { const u32x2 e = fetch(idx[data[4 * Q + k]]); rcp = e.x; pk = e.y; }
        o.step(x, live, rcp, pk, bits);
    }

    // (B) whole groups Q-1 .. 0; trip t covers groups Q-1-4t .. Q-4-4t = bytes [4 (Q-4t-4), 4 (Q-4t))
    const u32 npair = Q >> 3;                             // double trips
    const u32 ntrip = 2 * npair;
    if (wave_any(npair > 0)) {
        struct DT { u32x4 a, b; };                        // the pieces of trips 2j and 2j+1
        auto load_dt = [&](u32 j) -> DT {
            gcu8 *p = j < npair ? data + 4ull * (Q - 8 * j) - 32 : safe;
            DT r = {*(GAS const u32x4_unaligned *)(p + 16), *(GAS const u32x4_unaligned *)p};
            return r;
        };
        struct I4 { u32 c0, c1, c2, c3; };
        const u32 sh = 8 * k;
        auto idx4 = [&](u32x4 v) -> I4 {                  // steps run from the highest group (v.w) down
            I4 r = {idx[(v.w >> sh) & 0xff], idx[(v.z >> sh) & 0xff], idx[(v.y >> sh) & 0xff], idx[(v.x >> sh) & 0xff]};
            return r;
        };
        auto cum4 = [&](const I4 &c) -> u32x4 {
            u32x4 r = {pair(c.c0), pair(c.c1), pair(c.c2), pair(c.c3)};
            return r;
        };
        auto topk4 = [&](u32x4 p) -> u32x4 {
            u32x4 r = {topk(p.x), topk(p.y), topk(p.z), topk(p.w)};
            return r;
        };
        auto rcp4 = [&](u32x4 p) -> u32x4 {
            u32x4 r = {rcpof(p.x), rcpof(p.y), rcpof(p.z), rcpof(p.w)};
            return r;
        };
        I4 I2;
        u32x4 P0, Praw, R0;
        DT Q0, Q1, Q2, Q3;                                // piece pair j lives in Q[j % 4]
        {
            Q0 = load_dt(0); Q1 = load_dt(1); Q2 = load_dt(2); Q3 = load_dt(3);
            const I4 i0 = idx4(Q0.a), i1 = idx4(Q0.b);
            I2 = idx4(Q1.a);
            P0 = topk4(cum4(i0));
            Praw = cum4(i1);
            R0 = rcp4(P0);
        }
        u32 t = 0;
        auto trip = [&](u32x4 wnext3) {
            const bool live = t < ntrip;
            const I4 In = idx4(wnext3);                   // bytes of trip t+3
            const u32x4 Pn = cum4(I2);                    // pairs of trip t+2
            const u32x4 P1 = topk4(Praw);                 // trip t+1, read during the previous trip
            const u32x4 Rn = rcp4(P1);
            __builtin_amdgcn_sched_barrier(0);
            o.step(x, live, R0.x, P0.x, bits);
            o.step(x, live, R0.y, P0.y, bits);
            o.step(x, live, R0.z, P0.z, bits);
            o.step(x, live, R0.w, P0.w, bits);
            I2 = In; P0 = P1; Praw = Pn; R0 = Rn;
            t++;
            __builtin_amdgcn_sched_barrier(0);
        };
        for (u32 d = 0; wave_any(d < npair); d += 4) {
            Q0 = load_dt(d + 4); o.flush_pipelined(); trip(Q1.b); trip(Q2.a);
            Q1 = load_dt(d + 5); o.flush_pipelined(); trip(Q2.b); trip(Q3.a);
            Q2 = load_dt(d + 6); o.flush_pipelined(); trip(Q3.b); trip(Q0.a);
            Q3 = load_dt(d + 7); o.flush_pipelined(); trip(Q0.b); trip(Q1.a);
        }
        o.flush_drain();
        o.flush();
    }
    // (B') the groups below the pipelined trips, one step each
    for (u32 g = Q - 4 * ntrip; wave_any(g > 0); ) {
        const bool live = g > 0;
        u32 rcp = 0, pk = 0;
        if (live) { g--; const u32x2 e = fetch(idx[data[4 * g + k]]); rcp = e.x; pk = e.y; }
        o.step(x, live, rcp, pk, bits);
        o.flush();
    }
    return o.finish(x);
}


// ---------------------------------------------------------------------------------------------
// k_enc_chain: QPW streams per wave, one launch per LDS size class (see k_dec_chain).
// ---------------------------------------------------------------------------------------------
// LDS_IMG: a workgroup of up to four waves shares one LDS copy of the reciprocal table; each quad
// owns lds_per_item bytes (image, then the word ring).  Waves never meet again after the set-up.
// PK: the class holds packed order-1 streams only (10-bit tables): a 1,025-entry reciprocal table suffices.
// FT: the class holds packed streams of the short-index kind: the frequency table in place of the reciprocals.
// aff_on (option enc_affine): waves of the short-index kind whose streams all have affine alphabets (EncItem.affine) take
// the pipelined loop's affine body; aff_count: where they count their streams for the route read-out (nullptr: not kept).
#define ENC_LRCP_PK_BYTES 4112u      // 1,025 dwords, padded to 16
template <bool LDS_IMG, bool PK, bool FT = false>
__global__ __launch_bounds__(256) void k_enc_chain(EncItem *items, const u32 *rcptab_, u8 *dump_, const u32 *list, u32 *count,
                                                   int qpw, int spw, u32 lds_per_item, int dyn, int aff_on, u32 *aff_count)
{
    extern __shared__ __attribute__((aligned(16))) u8 lds[];
    const u32 tid = threadIdx.x;
    const u32 lane = tid & (WAVE - 1);
    // qpw streams per workgroup, spw per wave (the first spw quads of each wave)
    const u32 wq = lane >> 2;
    const u32 quad = (tid >> 6) * (u32)spw + wq;
    // persistent: as many workgroups as are resident at once, each walking shares of its class's list (see k_dec_chain
    // and r4x16_sched.h: longest streams first, shares claimed from the class's counter, count[SCHED_SEATS] workgroups work)
    const int nmine = (int)count[SCHED_COUNT];
    list += count[SCHED_START];
    SchedWalk walk(count, nmine, qpw, dyn != 0);
    for (;;) {
    const int wg = LDS_IMG ? walk.next_wg((volatile u32 *)lds + 1) : walk.next_wave();
    if (wg < 0) break;
    const int slot = wg * qpw + (int)quad;
    const bool mine = wq < (u32)spw && quad < (u32)qpw && slot < nmine;
    EncItem *I = &items[mine ? list[slot] : list[wg * qpw]];
    bool active = mine && I->active;
    const u32 img_bytes = active ? I->img_bytes : 0u;
    if (LDS_IMG) {
        // workgroup-wide "does anybody have work here" through one dword of the dynamic LDS
        // (__syncthreads_or would bring 256 bytes of static LDS with it: one stream's worth of room)
        volatile u32 *flag = (volatile u32 *)lds;
        if (tid == 0) *flag = 0;
        __syncthreads();
        if (active) *flag = 1;
        __syncthreads();
        const u32 any = *flag;
        __syncthreads();
        if (!any) continue;
    } else if (!wave_any(active)) continue;
    sched_setprio(sched_prio_of(active, active ? I->n : 0u));

    const u32 order = active ? I->order : 2u;
    gcu32 *rcptab = to_global(rcptab_);
    gcu8 *data = (gcu8 *)I->data;
    gu8 *send = (gu8 *)I->scratch_end;
    const u32 n = I->n, ns = I->ns, bits = active ? I->bits : 12u;
    u32 pay;
    if (LDS_IMG) {
        u32 *lrcp = (u32 *)lds;                            // FT: LDS address 0, which chain_encode_o1_lds' rcpof relies on
        u8 *slots = lds + (FT ? ENC_LFREQ_BYTES : PK ? ENC_LRCP_PK_BYTES : ENC_LRCP_BYTES);
        if (FT) for (u32 j = tid; j < 2u * ENC_FREQTAB_ENTRIES; j += blockDim.x) lrcp[j] = rcptab[ENC_FREQTAB_OFF + j];
        else for (u32 j = tid; j < (PK ? 1025u : RCPTAB_ENTRIES); j += blockDim.x) lrcp[j] = rcptab[j];
        // each wave copies the images of its own quads (16-byte pieces)
        const u64 my_img = active ? I->image : 0ull;
        const u32 wq0 = (tid >> 6) * (u32)spw;             // first stream slot of this wave
        for (u32 qd = 0; qd < WAVE / 4; qd++) {
            const u64 src = __shfl(my_img, (int)qd * 4);
            const u32 nb = __shfl(img_bytes, (int)qd * 4);
            if (!src) continue;
            gcu32x4 *s = (gcu32x4 *)src;
            u32x4 *dd = (u32x4 *)(slots + (u64)(wq0 + qd) * lds_per_item);
            for (u32 j = lane; j < ((nb + 15) >> 4); j += WAVE) dd[j] = s[j];
        }
        __syncthreads();
        // lanes without a stream read and write the LDS of stream 0 (nothing of theirs is ever used)
        const u32 slot = active ? quad : 0u;
        const u8 *im = slots + (u64)slot * lds_per_item;
        u8 *ring = slots + (u64)slot * lds_per_item + (lds_per_item - ENC_RING_BYTES);
        gu8 *dump = to_global(dump_) + 16u * ((blockIdx.x * blockDim.x + tid) & (ENC_DUMP_BYTES / 16u - 1u));
        if (FT) {
            // (a lane without a stream has no say; the same rule as k_enc_chain_rec's and the decoder's affine body)
            const u32 aff = !aff_on ? 0u : active ? I->affine : 1u;
            const bool aff_wave = !wave_any(aff == 0u);
            pay = chain_encode_o1_lds<PK, false, FT>(im, ring, lrcp, data, n, ns, bits, (gcu8 *)rcptab, send, dump, order == 1, lane, aff_wave, aff);
            const u32 nstreams = (u32)__popcll(__ballot(active) & 0x1111111111111111ull);
            if (aff_count && aff_wave && lane == 0) atomicAdd(aff_count, nstreams);
        } else pay = chain_encode_o1_lds<PK, false, FT>(im, ring, lrcp, data, n, ns, bits, (gcu8 *)rcptab, send, dump, order == 1, lane);
        if (!PK) pay |= chain_encode_o0_pipe(im, ring, lrcp, data, n, bits, (gcu8 *)rcptab, send, dump, order == 0, lane);
    } else {
        gcu8 *im = (gcu8 *)I->image;
        pay = chain_encode<1>(data, n, im, ns, bits, rcptab, send, order == 1, lane);
        pay |= chain_encode<0>(data, n, im, ns, bits, rcptab, send, order == 0, lane);
    }
    if (active && (lane & 3) == 0) I->pay_len = pay;
    if (LDS_IMG) __syncthreads();                          // LDS is reused by the next share
    }
    walk.leave();
}

