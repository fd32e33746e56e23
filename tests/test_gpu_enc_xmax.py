"""The encode chain's packed-row step with x_max taken from the row by one multiply and the renormalisation written
out per trip (htscodecs_amd/csrc/r4x16_enc_chain.h: chain_encode_o1_lds' topk / rcpof, EncOutT::trip_freq) against the
CPU oracle, byte for byte.

rans4x16_hip_compress_dev with order 1 and the symbol records off, exactly as tests/test_gpu_enc_affine.py calls it.
The inputs are runs of byte values from 33 on (46 symbols with byte 0, fewer in blocks too short to hold them) whose
count matrix holds the three pairs at which the new arithmetic could go wrong:
  * a context with a single successor: frequency 1,024, the widest a 10-bit table has - x_max = 2^31, bit 31 of the
    product, the table's last entry;
  * a pair that occurs exactly once: the narrow end;
  * the last symbol in the last context: the 32 bits that hold its pair reach beyond the row's fields, so the
    multiply's upper bits - its operand's sign among them - are not the image's own.
Every case asserts the route: packed rows of the short-index kind ("packed_freq") and the streams counted by waves of
the affine body ("packed_affine")."""
import numpy as np
import pytest

from test_enc_affine_cpu import affine_of, alpha_of
from test_gpu_enc_affine import SHORT as AFFINE_SHORT, check
from test_gpu_enc_step import takes_packed

# 1, 2, 3, 4, 5 and 9 double trips of the pipelined loop with every residue of the tail (36 .. 295 bytes); then the
# same behind 8,192 bytes (256 double trips: a whole number of unrolled passes)
SHORT = [n for n in AFFINE_SHORT if n >= 36]
LENGTHS = SHORT + [8192 + n for n in SHORT]


def block(n, seed=0, gap=False):
    """n bytes over the run 33 .. 33 + k - 1, k = min(45, n - 2) byte values, every one of them present:
    S = 33 occurs once and is followed by T = 34 (a context with a single successor), L = the run's last byte follows
    itself (the last symbol in the last context), and the rest is a permutation of the other values and then uniform
    draws from all but S.  The four bytes S T L L stand at a place the seed picks.  gap: one value of the middle is
    left out (and k is one more), which makes the alphabet no run."""
    k = min(45, n - 2) + (1 if gap else 0)
    a = np.arange(33, 33 + k, dtype=np.uint8)
    if gap:
        a = np.delete(a, k // 2)
        k -= 1
    S, T, L = a[0], a[1], a[-1]
    rng = np.random.default_rng(104729 * n + 17 * seed + (1 if gap else 0))
    rest = np.concatenate([rng.permutation(a[1:-1]), a[1:][rng.integers(0, k - 1, size=n - (k - 2) - 4)]])
    at = int(rng.integers(1, len(rest)))
    return np.concatenate([rest[:at], [S, T, L, L], rest[at:]]).astype(np.uint8).tobytes()


def counts(raw):
    """the order-1 pair counts F[context][symbol] of the bytes themselves"""
    a = np.frombuffer(raw, dtype=np.uint8).astype(np.int64)
    F = np.zeros((256, 256), dtype=np.int64)
    np.add.at(F, (a[:-1], a[1:]), 1)
    return F


def is_affine(raw):
    return affine_of(alpha_of(raw), 0 in raw) != 0


@pytest.fixture(scope="module")
def H():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import htscodecs_amd
    htscodecs_amd.load()
    return htscodecs_amd


@pytest.mark.gpu
@pytest.mark.parametrize("enc_affine", [1, 0], ids=["affine", "look-up"])
def test_every_length_alone(H, opts, enc_affine):
    """One block per call: one quad is live, every other lane of the wave codes neutral symbols (x_max = 2^31, the
    table's last entry) all the way."""
    for n in LENGTHS:
        check(H, opts, [block(n)], enc_affine, enc_affine)


@pytest.mark.gpu
@pytest.mark.parametrize("enc_affine", [1, 0], ids=["affine", "look-up"])
@pytest.mark.parametrize("nblk", [13, 9])
def test_full_wave_beside_a_partly_filled_wave(H, opts, nblk, enc_affine):
    """A small batch's workgroups are one wave of eight streams: 13 blocks are a full wave beside a wave of five, 9
    blocks a full wave beside a wave with one stream."""
    for n in (4 * (8 * 9 + 1) + 2, 8192 + 4 * (8 * 5 + 1) + 3):
        check(H, opts, [block(n, seed=i) for i in range(nblk)], nblk * enc_affine, enc_affine)


@pytest.mark.gpu
@pytest.mark.parametrize("enc_affine", [1, 0], ids=["affine", "look-up"])
def test_mixed_lengths_in_one_wave(H, opts, enc_affine):
    """1, 3 and 9 double trips - and the same behind 8,192 bytes - in one wave: streams end at different trips, and a
    lane past its end goes on with neutral symbols while its neighbours emit."""
    for far in (0, 8192):
        lens = [far + 4 * (8 * p + 1) + t for p, t in ((1, 0), (3, 1), (9, 2), (9, 3), (3, 3), (1, 2), (9, 0))]
        raws = [block(n, seed=5 + i) for i, n in enumerate(lens)]
        check(H, opts, raws, len(raws) * enc_affine, enc_affine)


@pytest.mark.gpu
def test_gapped_alphabet_takes_the_look_up_body(H, opts):
    """The same blocks with a byte value missing from the middle of the run: the look-up body of the same kernel, alone
    and nine to a batch."""
    for n in LENGTHS:
        check(H, opts, [block(n, gap=True)], 0)
    for n in (4 * (8 * 9 + 1) + 2, 8192 + 4 * (8 * 5 + 1) + 3):
        check(H, opts, [block(n, seed=i, gap=True) for i in range(9)], 0)


def test_cases_are_what_they_claim():
    """No GPU: the lengths' stages, and the three pairs in every block's count matrix."""
    assert {((n >> 2) - 1) >> 3 for n in SHORT} == {1, 2, 3, 4, 5, 9} and min(SHORT) == 36 and max(SHORT) == 295
    assert {n & 3 for n in SHORT} == {0, 1, 2, 3}
    assert {(((n >> 2) - 1) >> 3) - 256 for n in LENGTHS if n >= 8192} == {1, 2, 3, 4, 5, 9}
    blocks = [(block(n, seed, gap), n, gap) for n in LENGTHS for seed, gap in ((0, False), (3, False), (0, True))]
    blocks += [(block(n, seed=i), n, False) for n in (4 * (8 * 9 + 1) + 2, 8192 + 4 * (8 * 5 + 1) + 3) for i in range(13)]
    for raw, n, gap in blocks:
        assert len(raw) == n
        alpha = alpha_of(raw)
        assert alpha[1] == 33 and len(alpha) == min(45, n - 2) + 1, n             # every value of the run, and byte 0
        assert is_affine(raw) != gap and max(raw) < 128, n
        assert takes_packed(raw), n
        F = counts(raw)
        S, L = alpha[1], alpha[-1]
        assert F[S].sum() == 1 and F[S, S + 1] == 1, n                            # one successor: frequency 1,024
        assert ((F == 1) & (F.sum(axis=1, keepdims=True) > 1)).any(), n           # a pair that occurs once, beside others
        assert F[L, L] >= 1, n                                                    # the last symbol in the last context
        # ... and a single successor is not the block's only kind of context
        assert ((F > 0).sum(axis=1) > 1).any(), n
