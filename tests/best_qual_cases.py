"""Inputs and expected results of the quality best-of tests across rANS 4x16, arith_dynamic and fqzcomp_qual
(test_best_qual_cpu.py, test_gpu_best_qual.py; include/rans4x16_hip.h part 2n).  The expectations come from the CPU alone,
each pinned to the reference by its own suite: cpu_libs.oracle() for rANS 4x16 and arith_enc_model.compress for
arith_dynamic (through best_any_cases), codec.fqz_pick_parameters + fqz_enc_model.compress for fqzcomp_qual,
fqz_best_cases.expect for that sub-list's result, and the cross rule of part 2n below.  No test lives here.

The small family (small_blocks): slices of 1, 2, 5 and 40 records of 1 .. 65 bytes over alphabets of 2, 5 and 41 qualities,
fqz_enc_model.drop_in_case(), and the sweeps - one record grown a byte at a time, which is where two codecs' sizes cross.
It has 105 blocks.  Under the three lists of LISTS its census (small_census) is, in (block, list) pairs: rANS 4x16 wins 23
outright, arith_dynamic 174, fqzcomp_qual 37; 46 ties of equal size involve the fqzcomp winner and 35 are ties between rANS
and arith alone."""
import functools
import random

import best_any_cases as A
import fqz_best_cases as B
import fqz_enc_model as E
import fqz_model as M
import fqz_pick_cases as P

CODEC_RANS, CODEC_ARITH, CODEC_MASK = A.CODEC_RANS, A.CODEC_ARITH, A.CODEC_MASK
CODEC_FQZ = 3 << 24
OK, CAPACITY, SIZE, UNSUPPORTED, EMPTY, UNDECIDED = A.OK, A.CAPACITY, A.SIZE, A.UNSUPPORTED, A.EMPTY, P.E_UNDECIDED
KINDS = ("blocks", "chunks", "rans", "arith", "fqz", "tie", "failed", "undecided")
rans, arith = A.rans, A.arith

RECORDS = (1, 2, 5, 40)
ALPHABETS = (2, 5, 41)


def fqz(strat):
    return CODEC_FQZ | strat


TRIPLE = (rans(0), arith(0), fqz(0))
EIGHT = (rans(1), rans(65), arith(1), arith(65), fqz(0), fqz(1), fqz(2), fqz(3))
LISTS = (TRIPLE, tuple(reversed(TRIPLE)), EIGHT)


def who_of(method):
    if method < 0:
        return "failed"
    return {CODEC_RANS: "rans", CODEC_ARITH: "arith", CODEC_FQZ: "fqz"}[method & CODEC_MASK]


def split(methods):
    """the three sub-lists, each in list order: [(position in the list, tagged method)] by codec name"""
    subs = {"rans": [], "arith": [], "fqz": []}
    for pos, m in enumerate(methods):
        subs[who_of(m)].append((pos, m))
    return subs


@functools.lru_cache(maxsize=None)
def _fqz_candidate(vers, strat, data, lens, flags):
    """(status, stream or None, lengths as the fix-ups leave them) of fqz_compress_pick under one strategy, on the CPU"""
    st, par, hl, hf = P.host_pick(vers, strat, data, list(lens), list(flags))
    if st == 0:
        st = E.verdict(data, hl, hf, par)
    return st, (E.compress(data, hl, hf, par) if st == 0 else None), (tuple(hl) if st == 0 else None)


def fqz_sub(block, strats, vers=4):
    """(status, stream or None, index into strats or -1, lengths out or None) of part 2l's call on the CPU"""
    data, lens, flags = block
    cands = [_fqz_candidate(vers, min(s, 4), bytes(data), tuple(lens), tuple(flags)) for s in strats]
    st, out, j = B.expect([(c[0], c[1]) for c in cands])
    return st, out, j, (list(cands[j][2]) if j >= 0 else None)


def cross(methods, results):
    """The cross rule.  results: {codec name: (status, stream or None, position of the winning method in `methods`)} for
    the codecs that have a sub-list.  -> (chosen tagged method or -1, stream or None, status, tie).  An undecided fqzcomp
    sub-list leaves the block undecided; otherwise the smallest stream among the sub-lists with status 0, on equal sizes the
    one whose winner stands earlier; with none, the status of the sub-list whose first method stands first.  tie: the
    smallest size is shared by two codecs' winners."""
    if "fqz" in results and results["fqz"][0] == UNDECIDED:
        return -1, None, UNDECIDED, False
    ok = sorted((len(out), pos, name) for name, (st, out, pos) in results.items() if st == OK)
    if not ok:
        return -1, None, results[who_of(methods[0])][0], False
    size, pos, name = ok[0]
    return methods[pos], results[name][1], OK, len(ok) > 1 and ok[1][0] == size


def expect(block, methods, vers=4, fqz_result=None):
    """(chosen, stream, status, tie, lengths out or None) of block (data, lens, flags) under the tagged list.  fqz_result:
    the fqzcomp sub-list's (status, stream, index, lengths) where the test knows it from elsewhere (the reference's own
    streams, an undecided pick)."""
    data = bytes(block[0])
    subs = split(methods)
    results = {}
    for name in ("rans", "arith"):
        if subs[name]:
            chosen, out, st, _ = A.expect(data, [m for pos, m in subs[name]])
            results[name] = (st, out, min(pos for pos, m in subs[name] if m == chosen) if st == OK else -1)
    lens_out = None
    if subs["fqz"]:
        st, out, j, lens_out = fqz_result if fqz_result is not None else fqz_sub(block, [m & ~CODEC_MASK for pos, m in subs["fqz"]], vers)
        results["fqz"] = (st, out, subs["fqz"][j][0] if j >= 0 else -1)
    chosen, out, st, tie = cross(methods, results)
    return chosen, out, st, tie, (lens_out if who_of(chosen) == "fqz" else None)


def census(blocks, methods, vers=4):
    """{route kind: count} of one call over `blocks` in one chunk, as R4X16_ROUTE_BEST_QUAL counts them"""
    out = dict.fromkeys(KINDS, 0)
    out["chunks"] = 1 if blocks else 0
    for b in blocks:
        chosen, _, st, tie, _ = expect(b, methods, vers)
        out["blocks"] += 1
        out["undecided" if st == UNDECIDED else who_of(chosen)] += 1
        out["tie"] += tie
    return out


# ---- the small family ----------------------------------------------------------------------------------------------------
def _walk(rng, n, nsym):
    """n qualities of an alphabet of nsym: a walk that mostly stays, as qualities do"""
    q, out = rng.randrange(nsym), bytearray()
    for _ in range(n):
        if rng.random() < 0.3:
            q = min(nsym - 1, max(0, q + rng.choice((-3, -1, 1, 2))))
        out.append(q)
    return bytes(out)


def _runs(rng, n, nsym, p):
    """n qualities in long runs: a new value with probability p - where the run-length order words of rANS 4x16 win"""
    q, out = rng.randrange(nsym), bytearray()
    for _ in range(n):
        if rng.random() < p:
            q = rng.randrange(nsym)
        out.append(q)
    return bytes(out)


def _draw(rng, n, nsym, kind):
    if kind == "walk":
        return _walk(rng, n, nsym)
    if kind == "runs":
        return _runs(rng, n, nsym, 0.01)
    return bytes(rng.randrange(nsym) for _ in range(n))


def _slice(rng, nrec, nsym, kind):
    lens = [rng.randrange(1, 66) for _ in range(nrec)]
    flags = [16 if rng.random() < 0.4 else 0 for _ in lens]
    return _draw(rng, sum(lens), nsym, kind), lens, flags


# one record grown a byte at a time: (alphabet, kind, seed, first length, one past the last, step).  The first is where
# rANS 4x16 and arith_dynamic tie (the smallest blocks), the next four where the sizes of arith_dynamic and fqzcomp_qual
# cross under [rans 0, arith 0, FQZ|0], the last where rANS 4x16's X_RLE | order 1 wins under the list of eight.
SWEEPS = ((2, "even", 1, 1, 8, 1), (5, "walk", 1, 205, 213, 1), (5, "walk", 1, 235, 251, 1), (41, "walk", 1, 214, 218, 1),
          (41, "walk", 1, 288, 297, 1), (41, "runs", 3, 8, 66, 3))


@functools.lru_cache(maxsize=None)
def small_blocks():
    """[(data, lens, flags)]: Random(11); per record count and alphabet a walk, an even draw and long runs, four more
    slices of 40 records, fqz_enc_model.drop_in_case(), the sweeps"""
    rng = random.Random(11)
    blocks = [_slice(rng, nrec, nsym, kind) for nrec in RECORDS for nsym in ALPHABETS for kind in ("walk", "even", "runs")]
    blocks += [_slice(rng, 40, nsym, "walk") for nsym in (5, 41, 5, 41)]
    blocks.append(E.drop_in_case())
    for nsym, kind, seed, lo, hi, step in SWEEPS:
        for n in range(lo, hi, step):
            blocks.append((_draw(random.Random(seed), n, nsym, kind), [n], [0]))
    return tuple((bytes(d), tuple(l), tuple(f)) for d, l, f in blocks)


@functools.lru_cache(maxsize=None)
def small_census():
    """Over the small family under LISTS, in (block, list) pairs: the wins of each codec with no other stream as small, the
    ties that involve the fqzcomp winner, the ties between rANS and arith alone.  At least 10, 10, 10, 5 and 5 are
    conditions, so that no direction and neither tie rule passes vacuously."""
    wins = dict(rans=0, arith=0, fqz=0)
    fqz_ties = ra_ties = 0
    for methods in LISTS:
        for b in small_blocks():
            chosen, out, st, tie, _ = expect(b, methods)
            assert st == OK, (st, len(b[0]), methods)
            if not tie:
                wins[who_of(chosen)] += 1
                continue
            f = fqz_sub(b, [m & ~CODEC_MASK for pos, m in split(methods)["fqz"]])
            if f[0] == OK and len(f[1]) == len(out):
                fqz_ties += 1
            else:
                ra_ties += 1
    got = (wins["rans"], wins["arith"], wins["fqz"], fqz_ties, ra_ties)
    assert min(got[:3]) >= 10 and fqz_ties >= 5 and ra_ties >= 5, got
    return got
