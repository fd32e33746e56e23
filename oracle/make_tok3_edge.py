#!/usr/bin/env python3
"""Make tests/golden/tok3/edge.bin and the table of README.edge.md: small name blocks, one per branch of the reference's
name tokeniser and side of it, with the containers the REFERENCE wrote for them (oracle/_ref/tok3_ref: the reference's
unchanged sources behind oracle/tok3_ref_driver.c, sanitizers on; `make -C oracle` builds it where a reference tree is).

Nothing of this project's tokeniser, model or kernel, has a say in what is written: the blocks are made here, the answers
are the driver's.  A case is kept only where the driver exits 0 with nothing on stderr (no sanitizer report) and the
reference decoded its own container back to the block's names; every case below is expected to be kept, and the script
exits non-zero if one is not.

    python oracle/make_tok3_edge.py            write the fixture and rewrite the table between the README's markers
    python oracle/make_tok3_edge.py --check    make everything again and compare with what is committed
"""
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tok3_edge_cases as X                                     # the fixture's layout and the random blocks

DRIVER = os.path.join(ROOT, "oracle", "_ref", "tok3_ref")
BEGIN, END = "<!-- table: begin (oracle/make_tok3_edge.py) -->", "<!-- table: end -->"
EVERY = ((1, 0), (7, 0), (7, 1))                                # (level, use_arith) of every case
LARGEST = ((3, 0), (5, 0), (9, 0))                              # and of the ten largest blocks


def lines(names, sep=b"\n", tail=b""):
    return b"".join(n + sep for n in names) + tail


# ---- the prefix rules (:632-670) -------------------------------------------------------------------------------------
def pacbio(lead, l, who, k):
    """A name the PacBio test reads as l bytes long: 'm' at d[f], '_' at d[7] and d[f + 14], '/' at d[f + 61]; who
    changes a byte inside the 60-byte prefix, k the bytes behind it."""
    f = 1 if lead == b">" else 0
    d = bytearray(b"m140415_143853_42175_c100635972550000001823121909121417_s1_p0" + b"xx")
    if f:
        d = bytearray(b">") + d
    d[f], d[7], d[f + 14], d[f + 61] = 109, 95, 95, 47
    d[20] = 48 + who
    d = bytes(d[:f + 62])
    rest = l - len(d)
    name = d + (b"%d/%d_%d" % (553 + k, 100 * k, 1234567 + k))[:rest].ljust(rest, b"7")
    assert len(name) == l
    return (b"@" if lead == b"@" else b"") + name


def ion(lead, l, who, k):
    """':' at d[f + 5] and d[f + 11], l bytes."""
    f = 1 if lead == b">" else 0
    head = (b">" if f else b"") + b"ABC%c%d:" % (68 + who, k % 2)
    name = head + b"%05d:" % (120 + k) + (b"%07d" % (77 * k + 5))[-(l - len(head) - 6):]
    assert len(name) == l and name[f + 5] == 58 and name[f + 11] == 58
    return (b"@" if lead == b"@" else b"") + name


def ont(lead, l, first, last, who, k):
    """A UUID (its first byte `first`, its 36th `last`) and what follows it, l bytes as the test counts them; who and k
    change bytes inside the UUID, so that the names differ at any l."""
    f = 1 if lead == b">" else 0
    uuid = bytearray(b"f33d30d5-6eb8-4115-8f46-154c2620a5df")
    uuid[0], uuid[35], uuid[3], uuid[30] = first, last, 48 + who, 48 + k
    name = ((b">" if f else b"") + bytes(uuid) + b"_B")[:l]
    assert len(name) == l
    return (b"@" if lead == b"@" else b"") + name


def interleave(make):
    """A(0) B(0) A(1) B(1) A(2): with the rule taken, A(1) is coded against A(0), two names back; without, against B(0)."""
    return [make(0, 0), make(1, 0), make(0, 1), make(1, 1), make(0, 2)]


def hand_cases():
    """[(name, branch, side, block)]"""
    out = []
    add = lambda name, branch, side, block: out.append((name, branch, side, bytes(block)))

    # token positions
    for end in (63, 64, 65, 126, 127):
        body = (b"a1" * 64)[:end - 1]
        side = {63: "one pass", 64: "the first name of the second pass (64 tokens and more)", 65: "second pass",
                126: "one below the last clean position", 127: "the last position the reference takes cleanly"}[end]
        add("n_end_%d" % end, "token position of N_END", side, lines([b"ab", body, body[:-1] + b"b", b"a2" + body[2:]]))
    pre = b"-" * 59
    runs = [b"123456789" * 11, b"123456789" * 5 + b"012345678" + b"123456790" * 5, b"123456789" * 10 + b"123456799"]
    add("digit_pieces_60_70", "token position of digit pieces", "tokens 60 to 70 are the 9-digit pieces of one run, across position 64",
        lines([pre + r for r in runs] + [pre + runs[0]]))

    # digits
    for w in (8, 9, 10, 17, 18, 19, 27):
        d = (b"123456789" * 3)[:w]
        pieces = "%d piece%s" % ((w + 8) // 9, "" if w <= 9 else "s") + ("" if w % 9 else ", the last one full")
        add("run_%d" % w, "digit run cut into pieces of 9 (:848, :899)", "%d digits: %s" % (w, pieces),
            lines([b"r" + d + b"x", b"r" + d[:-1] + b"8x", b"r" + d + b"y"]))
    add("value_999999999", "largest 9-digit value", "999999999, then one less and one more digit", lines([b"v999999999", b"v999999998", b"v9999999990"]))
    for w in (1, 2, 9, 10):
        z = b"0" * w
        add("zeros_%d" % w, "N_DIGITS0 of zeros (:842-892)", "%d zero%s%s" % (w, "" if w == 1 else "s", ": a full piece and one more" if w == 10 else ""),
            lines([z, b"q" + z, z, b"q" + z + b"1"]))
    add("digits0_met_same_width", "N_DIGITS0 met by a number without a leading zero (:916-919)", "same width: coded as N_DIGITS0",
        lines([b"x:007", b"x:123", b"x:124", b"x:380"]))
    add("digits0_met_other_width", "N_DIGITS0 met by a number without a leading zero (:916-919)", "another width: N_DIGITS",
        lines([b"x:007", b"x:1234", b"x:12", b"x:008"]))
    for what, a, b in (("0", b"0007", b"0007"), ("1", b"0007", b"0008"), ("255", b"0001", b"0256"), ("256", b"0001", b"0257"),
                       ("neg", b"0100", b"0099"), ("width", b"0007", b"00008")):
        side = {"0": "difference 0: N_MATCH", "1": "difference 1", "255": "difference 255: the last N_DDELTA0",
                "256": "difference 256: N_DIGITS0 again", "neg": "difference -1: N_DIGITS0 again", "width": "difference 1 at another width: N_DIGITS0 again"}[what]
        add("ddelta0_%s" % what, "N_DDELTA0 (:856-878)", side, lines([a + b"a", b + b"b", b + b"c"]))
    for what, a, b in (("0", 100, 100), ("1", 100, 101), ("255", 100, 355), ("256", 100, 356), ("neg", 100, 99)):
        side = {"0": "difference 0: N_MATCH", "1": "difference 1", "255": "difference 255: the last N_DDELTA",
                "256": "difference 256: N_DIGITS", "neg": "difference -1: N_DIGITS"}[what]
        add("ddelta_%s" % what, "N_DDELTA (:923-949)", side, lines([b"r%da" % a, b"r%db" % b, b"r%dc" % b]))
    add("wrap_999999999_3", "the difference as a signed number (:924)", "previous 999999999, current 3: negative, N_DIGITS", lines([b"v999999999", b"v3", b"v4"]))
    add("wrap_3_999999999", "the difference as a signed number (:924)", "previous 3, current 999999999: large, N_DIGITS", lines([b"v3", b"v999999999", b"v4"]))
    add("delta_rule_holds", "5 + dcount > icount (:934)", "icount 4, dcount 0: the last name is an N_DDELTA",
        lines([b"r %d" % v for v in (1000, 2000, 3000, 4000, 5000, 5001)]))
    add("delta_rule_fails", "5 + dcount > icount (:934)", "icount 5, dcount 0: the last two names are N_DIGITS",
        lines([b"r %d" % v for v in (1000, 2000, 3000, 4000, 5000, 6000, 6001, 6002)]))

    # alpha and char
    add("alpha_same_length", "N_ALPHA against the earlier stretch (:813-835)", "same length, other bytes", lines([b"abc1", b"abd1", b"abd2"]))
    add("alpha_same_bytes", "N_ALPHA against the earlier stretch (:813-835)", "the same bytes at another length", lines([b"abc1", b"abcd1", b"ab1", b"abc1x"]))
    add("alpha_punct", "an alpha stretch takes punctuation (:798)", "a letter, then punctuation and letters: one stretch", lines([b"ab:c_d-9", b"ab:c_d-8", b"a:9", b":a9"]))
    add("single_letter", "a stretch of one byte is an N_CHAR (:811)", "one letter between digits, and two", lines([b"1a2", b"1b2", b"1ab2", b"1a2x"]))
    for byte, side in ((0x0b, "0x0b: above the separators, no class: N_CHAR"), (0x1f, "0x1f: below the blank: N_CHAR"),
                       (0x20, "0x20: the blank is no punctuation: N_CHAR, ends a stretch"), (0x21, "0x21: the first punctuation byte: inside a stretch"),
                       (0x7e, "0x7e: the last punctuation byte: inside a stretch"), (0x7f, "0x7f: no punctuation: N_CHAR, ends a stretch")):
        c = bytes([byte])
        add("byte_%02x" % byte, "byte classes (isalpha / ispunct / isdigit, C locale)", side, lines([b"ab" + c + b"cd", b"ab" + c + b"ce", c, c + b"1" + c, b"ab" + c + b"cd9"]))

    # the prefix rules
    for lead, tag in ((b"", "plain"), (b"@", "at"), (b">", "gt")):
        for l in (70, 71):
            add("pacbio_%d_%s" % (l, tag), "PacBio: l > 70 (:636)", "l = %d, %s: %s" % (l, tag, "taken" if l > 70 else "not taken"),
                lines(interleave(lambda who, k: pacbio(lead, l, who, k))))
        for l in (16, 17, 18):
            add("ion_%d_%s" % (l, tag), "IonTorrent: l == 17 (:639)", "l = %d, %s: %s" % (l, tag, "taken" if l == 17 else "not taken"),
                lines(interleave(lambda who, k: ion(lead, l, who, k))))
        for what, l, first, last in (("37", 37, 102, 102), ("38", 38, 102, 102), ("first_g", 38, 103, 102), ("last_g", 38, 102, 103)):
            side = {"37": "l = 37: not taken", "38": "l = 38, 'f' as first and as 36th byte: taken", "first_g": "'g' as first byte: not taken",
                    "last_g": "'g' as 36th byte: not taken"}[what]
            add("ont_%s_%s" % (what, tag), "ONT: l > 37 and hex digits at both ends of the UUID (:643-645)", "%s, %s" % (side, tag),
                lines(interleave(lambda who, k: ont(lead, l, first, last, who, k))))
        ill = {"4": lambda who, k: b"HS2%d_09827:2:%d:%d:%d#49" % (who, 1101 + k, 1234 + 7 * k, 5678 + 300 * k),
               "3": lambda who, k: b"HS2%d_09827:%d:%d:%d#49" % (who, 1101 + k, 1234 + 7 * k, 5678 + 300 * k),
               "blank_behind": lambda who, k: b"HS2%d_09827:2:%d:%d:%d 1:N:0:ATCACG" % (who, 1101 + k, 1234 + 7 * k, 5678 + 300 * k),
               "blank_before": lambda who, k: b"HS2%d 09827:2:%d:%d:%d" % (who, 1101 + k, 1234 + 7 * k, 5678 + 300 * k)}
        for what, side in (("4", "four colons: taken"), ("3", "three colons: not taken"),
                           ("blank_behind", "a blank behind the four, colons behind the blank: taken, counted back from the blank"),
                           ("blank_before", "a blank in front of the fourth colon from the end: not taken")):
            add("illumina_%s_%s" % (what, tag), "Illumina: four colons in front of the first blank (:652-663)", "%s, %s" % (side, tag),
                lines(interleave(lambda who, k: lead + ill[what](who, k))))

    # the earlier name
    add("exact_longer", "exact hit in the trie (:710, :745)", "on a longer name: N_DIFF against it", lines([b"abc123", b"abc12", b"abc1", b"abc12"]))
    add("prefix_of_later", "exact hit in the trie (:710, :745)", "an earlier name is a prefix of this one: no hit", lines([b"abc1", b"abc12", b"abc123", b"abd"]))
    add("distance_0", "the name's own number as the earlier name (:700, :735)", "a fixed prefix no earlier name has: distance 0 behind the first name",
        lines([b"A:1:2:3:4", b"B:1:2:3:4", b"C:1:2:3:5", b"A:1:2:3:6"]))
    for dist in (1, 2, 255, 256, 999):
        add("dup_%d" % dist, "N_DUP and its distance (:745-754)", "distance %d" % dist, lines([b"X7"] + [b"b"] * (dist - 1) + [b"X7"]))
    add("all_same", "N_DUP and its distance (:745-754)", "every name the same", lines([b"same.1"] * 20))
    add("one_name", "a block of one name", "the one-byte switch column is dropped (:1417-1427)", lines([b"only:1"]))

    # the drop rule
    add("drop_with_value", "the drop rule (:1406-1429)", "all N_MATCH behind the first byte, a value column beside it: dropped", lines([b"ab1", b"ab2", b"ab3"]))
    add("drop_without_value", "the drop rule (:1406-1429)", "a one-byte type column with no value column (N_END of one name): kept", lines([b"ab"]))
    add("drop_not_all_match", "the drop rule (:1406-1429)", "another type behind the first byte: kept", lines([b"ab1", b"ab2", b"cd3", b"cd3x"]))

    # framing
    add("empty_front", "empty names (:1349-1380)", "in front", lines([b"", b"", b"a1", b"a2"]))
    add("empty_middle", "empty names (:1349-1380)", "in the middle", lines([b"a1", b"", b"", b"a2"]))
    add("empty_end", "empty names (:1349-1380)", "at the end", lines([b"a1", b"a2", b"", b""]))
    for sep in range(11):
        add("separator_%02x" % sep, "a name ends at any byte <= '\\n' (:1340, :1350)", "0x%02x" % sep, lines([b"one", b"two", b"one", b"t3"], sep=bytes([sep])))
    add("unterminated_tail", "the unterminated tail (:1352-1356)", "bytes behind the last separator: last_start in front of them", lines([b"r1", b"r2"], tail=b"r3 is cut"))
    add("terminated_tail", "the unterminated tail (:1352-1356)", "the block ends in a separator: last_start is its length", lines([b"r1", b"r2", b"r3 is cut"]))
    return out


CLASSES = ("letter", "1-9", "0", "punct", "other")


def byte_class(c):
    if 65 <= c <= 90 or 97 <= c <= 122:
        return 0
    if 49 <= c <= 57:
        return 1
    if c == 48:
        return 2
    return 3 if 33 <= c <= 126 else 4


def random_cases():
    """40 seeded random blocks of the kinds of tests/tok3_edge_cases.py, small: up to 24 names of up to 24 bytes, five of
    them with names of 65 to 120 tokens.  Between them every pair of neighbouring byte classes occurs."""
    rng = random.Random(2024)
    out, pairs = [], set()
    for k in range(40):
        if k % 7 == 6:
            block = X.random_block(rng, X.LONG, max_names=4, max_len=16)
        else:
            block = X.random_block(rng, X.PLAIN, max_names=24, max_len=24)
        for name in block.replace(b"\0", b"\n").replace(b"\x01", b"\n").split(b"\n"):
            pairs |= {(byte_class(a), byte_class(b)) for a, b in zip(name, name[1:])}
        out.append(("random_%02d" % k, "random names over a small alphabet", "seeded; %s" % ("names of 65 to 120 tokens among them" if k % 7 == 6 else "short names"), block))
    missing = [(CLASSES[a], CLASSES[b]) for a in range(5) for b in range(5) if (a, b) not in pairs]
    assert not missing, missing
    return out


def run_driver(block, wanted):
    """[(made, last_start, container, back)] per (level, use_arith) of `wanted`, or a string saying why not."""
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(src, "wb") as f:
            f.write(len(wanted).to_bytes(4, "little"))
            for level, use_arith in wanted:
                f.write(level.to_bytes(4, "little") + use_arith.to_bytes(4, "little") + len(block).to_bytes(4, "little") + block)
        r = subprocess.run([DRIVER, src, dst], capture_output=True, timeout=600)
        if r.returncode != 0 or r.stderr:
            return "exit status %d: %s" % (r.returncode, r.stderr.decode(errors="replace")[:400])
        with open(dst, "rb") as f:
            buf = f.read()
    u = lambda at: int.from_bytes(buf[at:at + 4], "little")
    assert u(0) == len(wanted)
    at, out = 4, []
    for _ in wanted:
        made, last_start, n = u(at), u(at + 4), u(at + 8)
        out.append((made, last_start, buf[at + 12:at + 12 + n], u(at + 12 + n)))
        at += 16 + n
    assert at == len(buf)
    return out


def make():
    todo = hand_cases() + random_cases()
    assert len({t[0] for t in todo}) == len(todo)
    largest = {t[0] for t in sorted(todo, key=lambda t: -len(t[3]))[:10]}
    cases, rows, lost = [], [], []
    for name, branch, side, block in todo:
        assert all(ch < 0x80 for ch in block), name
        wanted = EVERY + (LARGEST if name in largest else ())
        res = run_driver(block, wanted)
        if isinstance(res, str) or not all(made and back for made, _, _, back in res):
            lost.append((name, res if isinstance(res, str) else "not made or not decoded back"))
            continue
        vecs = tuple(X.Vector(lv, ua, ls, bytes(c)) for (lv, ua), (_, ls, c, _) in zip(wanted, res))
        cases.append(X.Case(name, block, vecs))
        nreads = sum(ch <= 10 for ch in block)
        rows.append("| `%s` | %s | %s | %d | %d | %s |" % (name, branch, side, nreads, len(block),
                                                       ", ".join("%d" % len(v.container) for v in vecs)))
    table = ["| case | branch | side | names | bytes | containers: rANS 1, rANS 7, arith 7 (and rANS 3, 5, 9) |", "|---|---|---|---|---|---|"] + rows
    return cases, "\n".join(table) + "\n", lost


def main():
    if not os.path.exists(DRIVER):
        sys.exit("no %s: make -C oracle builds it where a reference tree is" % DRIVER)
    cases, table, lost = make()
    for name, why in lost:
        print("NOT KEPT: %s: %s" % (name, why))
    with open(X.README) as f:
        text = f.read()
    head, rest = text.split(BEGIN)
    tail = rest.split(END)[1]
    new = head + BEGIN + "\n" + table + END + tail
    if "--check" in sys.argv[1:]:
        tmp = tempfile.mktemp()
        X.write(tmp, cases)
        with open(tmp, "rb") as f, open(X.EDGE, "rb") as g:
            same = f.read() == g.read()
        os.unlink(tmp)
        print("fixture %s, table %s" % ("same" if same else "DIFFERS", "same" if new == text else "DIFFERS"))
        sys.exit(1 if lost or not same or new != text else 0)
    X.write(X.EDGE, cases)
    with open(X.README, "w") as f:
        f.write(new)
    print("%d cases, %d vectors, %d bytes" % (len(cases), sum(len(c.vectors) for c in cases), os.path.getsize(X.EDGE)))
    sys.exit(1 if lost else 0)


if __name__ == "__main__":
    main()
