"""What the inputs of the arith GPU tests reach, counted by the Python model (arith_model.decode_core's census): every
event of the step, of the guards and of the run loop must occur at least twice in each place it can occur, over exactly
the stream lists the GPU tests decode (their cached builders are imported).  A kernel is only held to what its inputs
reach: thinning them fails here, on the CPU.  Also the coverage of the coder's input window - payload sizes, their
residues and the payload addresses mod 16 - and that the census changes nothing of what the model decodes."""
import collections
import functools

import arith_cases as K
import arith_model as M
import test_gpu_arith as A
import test_gpu_arith_hostile as Hs
import test_gpu_arith_trips as T

HOMES = ("o0", "o1_lds", "o1_global")
STEP = ("halve", "swap", "halve_swap", "halve_tie")                                     # every home and the run models
BOUNDARY = ("swap_boundary", "halve_swap_boundary", "halve_tie_boundary")               # symbol models only
GUARDS = ("range_lt_tot", "freq_gt_max", "ran_off", "starved")                          # every home and the run models
RUN_LOOP = ("ctx257", "chain3", "chain_cut", "run_clipped")


@functools.lru_cache(maxsize=None)
def lists():
    """{name: (streams, caps, planes, stripe_out)}: what each GPU test hands to the device call"""
    out = {}
    fx, raws = A.fixtures()
    out["fixtures"] = (fx, A._caps(fx, raws), 4, max(map(len, raws)))
    streams, raws = A.step_streams(), [r for _, r, _ in A.step_cases()]
    out["step"] = (streams, A._caps(streams, raws), 0, 0)
    for name, cases in (("edge damaged", Hs._sized([(s, c) for s, c, _ in K.edge()[1]])), ("model damaged", Hs._sized(K.model_damaged())),
                        ("global damaged", K.global_damaged())):
        out[name] = ([s for s, _ in cases], [c for _, c in cases], Hs.PLANES, Hs.STRIPE_OUT)
    streams, raws = K.tie_streams(), [r for _, r, _ in K.tie_cases()]
    out["ties"] = (streams, A._caps(streams, raws), 0, 0)
    streams, caps, _, _, _ = T.window_batch()
    out["window"] = (streams, caps, 0, 0)
    for name, (streams, raws), planes in (("many blocks", T.many_blocks(), 0), ("many planes", T.many_planes(), 4),
                                         ("wide stripes", T.wide_stripes(), 255), ("exact total", T.exact_total_blocks(), 4)):
        out[name] = (streams, [len(r) for r in raws], planes, max(map(len, raws)))
    for k, (streams, raws, planes) in enumerate(T.chunk_batches()):
        out["chunks %d" % k] = (streams, A._caps(streams, raws), planes, max(A._caps(streams, raws)))
    return out


@functools.lru_cache(maxsize=None)
def census():
    """{name: Counter} of the lists, each stream decoded once with the counter and compared with the plain model"""
    out = {}
    for name, (streams, caps, planes, stripe_out) in lists().items():
        ev = out[name] = collections.Counter()
        for s, cap in zip(streams, caps):
            got = M.uncompress_to(s, cap, max_planes=planes, max_stripe_out=stripe_out, events=ev)
            if name in ("ties", "global damaged", "exact total", "edge damaged"):       # (the census decodes what the model decodes)
                assert got == M.uncompress_to(s, cap, max_planes=planes, max_stripe_out=stripe_out), (name, s[:12].hex())
    return out


def _total():
    tot = collections.Counter()
    for ev in census().values():
        tot.update(ev)
    return tot


def test_every_event_is_reached_twice_wherever_it_can_occur():
    tot = _total()
    table = ["%-20s" % "event" + "".join("%11s" % w for w in HOMES + ("run",))]
    for e in STEP + BOUNDARY + GUARDS + ("short_start",) + RUN_LOOP:
        table.append("%-20s" % e + "".join("%11s" % (tot[w, e] if (w, e) in tot else "-") for w in HOMES + ("run",)))
    print("\n".join(table))
    need = [(w, e) for e in STEP + GUARDS for w in HOMES + ("run",)]
    need += [(w, e) for e in BOUNDARY + ("short_start",) for w in HOMES]
    need += [("run", e) for e in RUN_LOOP]
    short = [(w, e, tot[w, e]) for w, e in need if tot[w, e] < 2]
    assert not short, short


def test_the_lists_made_for_an_event_reach_it_themselves():
    """so that dropping one of them is noticed although another list happens to reach the same event"""
    c = census()
    for w in HOMES:
        assert c["ties"][w, "halve_tie"] >= 3 and c["ties"][w, "halve_tie_boundary"] >= 2, w
        assert c["ties"][w, "halve_swap"] >= 3 and c["ties"][w, "halve_swap_boundary"] >= 2, w
    assert c["ties"]["run", "halve_tie"] >= 2 and c["ties"]["run", "halve_swap"] >= 2
    assert len(lists()["global damaged"][0]) >= 60
    for e in GUARDS:
        assert c["global damaged"]["o1_global", e] >= 2, e
    for name in ("many blocks", "many planes"):
        assert c[name]["o1_global", "swap"] > 0, name


class CompareFirst(M.Model):
    """the model with the two halves of its update the other way round: the swap decided before the halving"""
    __slots__ = ()

    def _update(self, i):
        F, S = self.F, self.S
        F[i] += M.STEP
        self.tot += M.STEP
        swap = i > 0 and F[i] > F[i - 1]
        if self.tot > M.MAX_FREQ:
            for k in range(len(F)):
                F[k] -= F[k] >> 1
            self.tot = sum(F)
        if swap:
            F[i], F[i - 1] = F[i - 1], F[i]
            S[i], S[i - 1] = S[i - 1], S[i]


def _decode_plain(s, n, model):
    """decode_core's loop over a plain stream (flag byte, size, payload) with another model class"""
    flags, pos = s[0], 1 + M.var_get(s, 1, len(s))[0]
    m = s[pos] or 256
    models = [model(m) for _ in range(256 if flags & 1 else 1)]
    runs = [model(4) for _ in range(258)]
    rc = M.Decoder(s, pos + 1, len(s))
    out, last = bytearray(), 0
    while len(out) < n:
        last = rc.symbol(models[last if flags & 1 else 0])
        out.append(last)
        if flags & M.X_RLE:
            run, rctx = 0, last
            while True:
                r = rc.symbol(runs[rctx])
                rctx = M._run_ctx(rctx, last)
                run += r
                if not (r == 3 and run < n):
                    break
            out += bytes([last]) * min(run, n - len(out))
    return bytes(out)


def test_a_decoder_that_compares_before_it_halves_fails_every_tie_stream_and_no_twin():
    """the inputs tell the two orders apart, and only where they should: from the tie step on, in the last bytes"""
    for (what, raw, order), s in zip(K.tie_cases(), K.tie_streams()):
        assert _decode_plain(s, len(raw), M.Model) == raw, what
        got = _decode_plain(s, len(raw), CompareFirst)
        if "twin" in what:
            assert got == raw, what
        else:
            first = next(i for i in range(len(raw)) if got[i] != raw[i])
            assert len(raw) - 40 <= first, (what, first, len(raw))


def test_the_window_list_has_every_size_residue_and_alignment():
    streams, caps, raws, in_off, facts = T.window_batch()
    ev = census()["window"]
    for home in HOMES:
        sizes = {k[2] for k in ev if k[0] == home and k[1] == "payload"}
        assert sizes >= set(K.WINDOW_SIZES), (home, sorted(set(K.WINDOW_SIZES) - sizes))
        # valid streams (the model gives the raw input back) above 1,040 bytes of payload: every residue mod 16
        valid = [(size, at) for (h, size, at), s, cap, raw in zip(facts, streams, caps, raws) if h == home and raw is not None and size > 1040]
        assert all(M.uncompress_to(s, cap) == (0, raw) for s, cap, raw in zip(streams, caps, raws) if raw is not None)
        assert {size % 16 for size, _ in valid} == set(range(16)), home
        # the payload's address mod 16 (the input arena is aligned), among the payloads above 1 KiB
        assert {at for h, size, at in facts if h == home and size > 1024} == set(range(16)), home
    # what the record of sizes says is what the layout was made from
    assert collections.Counter((h, size) for h, size, _ in facts) == collections.Counter((k[0], k[2]) for k in ev.elements() if k[1] == "payload")
    base = {h: size for h, _, _, size in K.window_bases()}
    assert all(base[h] > 2100 for h in HOMES)
