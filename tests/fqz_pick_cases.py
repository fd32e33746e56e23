"""What the tests of the device pick share (test_fqz_pick_dev_cpu.py, test_gpu_fqz_pick.py): the reference-made cases of
tests/golden/fqzcomp/pick.bin (README.pick.md), the generator of its hashed inputs, the 16 fixtures as pick inputs, and
the host pick's answers, computed once per slice."""
import hashlib
import os
import struct

import numpy as np

import fqz_enc_model as E
import fqz_model as M

PICK = os.path.join(M.GOLDEN, "pick.bin")
E_UNDECIDED = 10
KINDS = ("blocks", "sel", "split", "dedup", "undecided", "host")
# the two cases whose ptab the reference's own read_array cannot read back (README.pick.md): parameter bytes that the
# header walk, the model and the encoder's front end refuse with E_TABLE, as they refuse them in a stream.  With
# nrec0_bytes they are the cases whose stream the reference did not decode back: the fixture keeps no stream for them.
UNREADABLE = ("first_len725", "first_len1448")
NOT_DECODED_BACK = UNREADABLE + ("nrec0_bytes",)


def lcg_bytes(seed, n, nsym):
    """README.pick.md's generator: x <- (1103515245 x + 12345) mod 2^31 from x = seed, byte k = (x_{k+1} >> 16) mod nsym.
    Vectorised: x_k = a^k x_0 + c (a^(k-1) + .. + 1), the powers and their sums in 64-bit wrap-around arithmetic."""
    a = np.full(n, 1103515245, dtype=np.uint64)
    with np.errstate(over="ignore"):
        pw = np.cumprod(a)                                           # a^1 .. a^n mod 2^64
        sums = np.cumsum(np.concatenate((np.ones(1, dtype=np.uint64), pw[:-1])))          # 1 + a + .. + a^(k-1)
        x = (pw * np.uint64(seed) + np.uint64(12345) * sums) & np.uint64((1 << 31) - 1)
    return ((x >> np.uint64(16)) % np.uint64(nsym)).astype(np.uint8).tobytes()


class Case:
    """name, vers, strat, lens, flags, size, data (None above 4 KiB until made from seed / nsym), digest, params, stream
    (None where not kept), stream_len / stream_digest (where the stream is kept as a hash)"""

    def bytes(self):
        if self.data is None:
            self.data = lcg_bytes(self.seed, self.size, self.nsym)
            assert hashlib.sha256(self.data).digest() == self.digest, self.name
        return self.data


_cases = []


def cases():
    if not _cases:
        raw = open(PICK, "rb").read()
        assert raw[:8] == b"FQPICK1\n"
        pos = 8
        def take(fmt):
            nonlocal pos
            v = struct.unpack_from("<" + fmt, raw, pos)
            pos += struct.calcsize("<" + fmt)
            return v
        def blob(n):
            nonlocal pos
            pos += n
            return raw[pos - n:pos]
        for _ in range(take("I")[0]):
            c = Case()
            c.name = blob(take("H")[0]).decode()
            c.vers, c.strat, nrec = take("3I")
            c.lens, c.flags = list(take("%dI" % nrec)), list(take("%dI" % nrec))
            c.size, kept = take("IB")
            c.data = c.digest = c.seed = c.nsym = None
            if kept:
                c.data = blob(c.size)
            else:
                c.digest = blob(32)
                c.seed, c.nsym = take("2I")
            c.params = blob(take("I")[0])
            kind = take("B")[0]
            c.stream = c.stream_len = c.stream_digest = None
            if kind == 1:
                c.stream = blob(take("I")[0])
            elif kind == 0:
                c.stream_len = take("I")[0]
                c.stream_digest = blob(32)
            _cases.append(c)
        assert pos == len(raw)
    return _cases


def small_cases():
    """the cases whose input bytes are kept (up to 4 KiB)"""
    return [c for c in cases() if c.digest is None]


def kept_cases():
    """the cases that carry the reference's stream: input bytes kept, and the stream decoded back by the reference"""
    return [c for c in cases() if c.stream is not None]


def reached(lens, size):
    """how many records the reference's encode loop reaches: those that start in front of the last byte"""
    n, pos = 0, 0
    for l in lens:
        if pos >= size:
            break
        n, pos = n + 1, pos + l
    return n


def fixture_inputs():
    """[(name, vers, strat, data, lens, flags, the reference's stream)] of the 16 streams"""
    return [(fn, 4, strat, data, lens, flags, stream) for fn, strat, stream, data, lens, flags in E.fixture_slices()]


_host = {}


def host_pick(vers, strat, data, lens, flags):
    """(status, parameter bytes, lens, flags) of rans4x16_hip_fqz_pick_parameters, computed once"""
    key = (vers, strat, bytes(data), tuple(lens), tuple(flags))
    if key not in _host:
        from htscodecs_amd import codec
        _host[key] = codec.fqz_pick_parameters(data, lens, flags, vers, strat)
    return _host[key]


def pflags_of(par):
    """pflags of the one parameter block: behind version and gflags, [max_sel and the selector table - store_array of 256
    zeros: the run lengths 255 and 1] and the two bytes of the starting context"""
    pos = 2
    if par[1] & M.GFLAG_HAVE_STAB:
        assert par[3:5] == bytes([255, 1])
        pos = 5
    return par[pos + 2]


def split_of(vers, strat, data, lens, flags):
    """whether the host pick takes the READ1 / READ2 split on this slice: the same slice without its READ2 flags gets the
    same average-quality decision (the bins are counted over both directions) and no split (no READ2 record: every term
    of that question is 0), so the split was taken where the selectors of the two picks differ"""
    with_r2 = host_pick(vers, strat, data, lens, flags)
    without = host_pick(vers, strat, data, lens, [f & ~128 for f in flags])
    assert with_r2[0] == without[0] == 0
    return 1 if [f >> 16 for f in with_r2[3]] != [f >> 16 for f in without[3]] else 0


def census(vers, blocks):
    """the route kinds of a batch of decided blocks [(strat, data, lens, flags)] from the host pick's answers"""
    out = dict.fromkeys(KINDS, 0)
    for strat, data, lens, flags in blocks:
        pflags = pflags_of(host_pick(vers, strat, data, lens, flags)[1])
        out["blocks"] += 1
        out["sel"] += 1 if pflags & M.PFLAG_DO_SEL else 0
        out["dedup"] += 1 if pflags & M.PFLAG_DO_DEDUP else 0
        out["split"] += split_of(vers, strat, data, lens, flags)
    return out
