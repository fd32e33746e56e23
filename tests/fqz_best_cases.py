"""What the tests of fqzcomp_qual's best-of-several calls share (test_fqz_best_cpu.py, test_gpu_fqz_best.py): the four
fixture slices with the reference's stream under each strategy, the winners' table, the pairs of
tests/golden/fqzcomp/pick.bin that share one slice, and the rule that makes a block's result out of its candidates'."""
import fqz_enc_model as E
import fqz_model as M
import fqz_pick_cases as P

# the slices in the order of the table, and per slice the strategy whose reference-made stream is smallest, with its size
SLICES = ("q4", "q40+dir", "q8", "qvar")
WINNERS = {"q4": (0, 9307), "q40+dir": (1, 43803), "q8": (0, 30012), "qvar": (3, 32073)}
PAIRS = ("qa4_r2taken", "qa0_r2taken", "qa4_r2refused", "qa0_r2refused")
LISTS = ([0, 1, 2, 3], [2, 0], [3, 1], [4, 0])


def _fixtures():
    return {fn: (strat, stream, data, lens, flags) for fn, strat, stream, data, lens, flags in E.fixture_slices()}


def fixture_slice(name):
    """(data, lens, flags) of a slice: the same under every strategy"""
    got = [_fixtures()["%s.%d" % (name, s)][2:] for s in range(4)]
    assert all(g == got[0] for g in got), name
    return got[0]


def fixture_stream(name, strat):
    return _fixtures()["%s.%d" % (name, strat)][1]


def pairs():
    """[(the `_s0` case, the `_s1` case)] of the pairs whose inputs, lengths and flags are identical"""
    by_name = {c.name: c for c in P.small_cases()}
    return [(by_name[n + "_s0"], by_name[n + "_s1"]) for n in PAIRS]


def max_sym(blocks):
    return max([max(bytes(b[0])) for b in blocks if len(b[0])] + [1])


def expect(cands):
    """(status, bytes, index) of a block from [(status, bytes or None)] of its candidates in list order: a candidate the
    pick cannot decide leaves the block undecided, one refused as unsupported (the slice is above the limits, or there
    was no room) fails the block, the smallest of the accepted ones wins - the first of equals - and with none left the
    block has the first candidate's status"""
    if any(st == P.E_UNDECIDED for st, out in cands):
        return P.E_UNDECIDED, None, -1
    if any(st == M.E_UNSUPPORTED for st, out in cands):
        return M.E_UNSUPPORTED, None, -1
    ok = [(len(out), j) for j, (st, out) in enumerate(cands) if st == 0]
    if not ok:
        return cands[0][0], None, -1
    size, j = min(ok)
    return 0, cands[j][1], j
