#!/usr/bin/env python3
"""Instruction mix of the hot-loop bodies in build/asm/*.s (made by `make -C htscodecs_amd/csrc asm`).
usage: tools/isa_count.py <kernel-name-substring> [block-label-substring]
       tools/isa_count.py --json <out>     the hot bodies' counts (and, for the decode chain on packed rows, the number of
                                           instructions in the shadow of each step's group read and head read, and the
                                           instructions of one 16-step trip from loop header to back edge, trip_path, and of
                                           what it issues between its last step's fence and the next trip's first wait:
                                           trip_tail)"""
import re
import sys
from collections import Counter

def blocks_of(src, name):
    i = src.index(name + ':')
    j = src.index('.Lfunc_end', i)
    blocks, cur, lab = [], [], 'entry'
    for l in src[i:j].split('\n'):
        if re.match(r'^\.LBB\d+_\d+:', l):
            blocks.append((lab, cur)); cur = []; lab = l.strip()
        elif l.strip() and not l.strip().startswith(('.', ';')):
            cur.append(l.strip())
    blocks.append((lab, cur))
    return blocks

HOT = {   # kernel-name mangled prefix -> (label, instruction that occurs once per step in the hot body[, its least steps: 4])
    # (the body of sixteen steps, which holds its own loop control and store: the bodies of eight behind it finish a stream)
    "_Z11k_dec_chainILb1ELi1ELi8EE": ("k_dec_chain<true,1>", "v_lshrrev_b64", 16),
    "_Z11k_dec_chainILb1ELi6ELi8EE": ("k_dec_chain<true,6>", "v_lshrrev_b64"),
    # the packed rows: the short-index kind with the frequency table (what the headline's quality blocks run on; the
    # label bench.py looks up), and the kind with the full index
    "_Z11k_enc_chainILb1ELb1ELb1EE": ("k_enc_chain<true,true>", "ds_write_b16"),
    "_Z11k_enc_chainILb1ELb1ELb0EE": ("k_enc_chain<true,true,false>", "ds_write_b16"),
    "_Z15k_enc_chain_rec": ("k_enc_chain_rec", "ds_write_b16"),
}


def shadows(b, first, second=None):
    """For each `first` in the block (a read on the step's dependent path; `second`: the read that completes it, taken
    where it follows within four instructions), the number of instructions issued between the read and the s_waitcnt
    that waits for it: what the step issues in the read's shadow.  LDS operations return in order, so a wait for
    lgkmcnt(c) covers the read once no more than c LDS operations were issued behind it; earlier waits (for reads
    issued before it) and s_nop are not counted as work.  A read whose wait lies in another block (the look-up that
    the loop header holds) is left out."""
    out = []
    for i, x in enumerate(b):
        if x.split()[0] != first:
            continue
        j = i
        if second:
            for k in range(i + 1, min(i + 5, len(b))):
                if re.match(second, b[k]):
                    j = k
                    break
        behind, work = j - i, 0                  # LDS operations issued behind `first`
        for k in range(j + 1, len(b)):
            op = b[k].split()[0]
            if op == 's_waitcnt':
                m = re.search(r'lgkmcnt\((\d+)\)', b[k])
                if m and int(m.group(1)) <= behind:
                    out.append(work)
                    break
            elif op.startswith('ds_'):
                behind += 1; work += 1
            elif op != 's_nop':
                work += 1
    return out


def cfg_of(src, name):
    """The function cut into basic blocks at labels and branches: the instructions, label -> index of its first
    instruction, block start -> next block's start, and the successors of a block with some lane live
    (s_cbranch_execz falls through and s_cbranch_execnz is taken, so the code under a lane mask counts)."""
    i = src.index(name + ':')
    ins, label_at = [], {}
    for l in src[i:src.index('.Lfunc_end', i)].split('\n'):
        lm = re.match(r'^(\.LBB\d+_\d+):', l)
        if lm:
            label_at[lm.group(1)] = len(ins)
        elif l.strip() and not l.strip().startswith(('.', ';')):
            ins.append(l.strip())
    starts = sorted(set(label_at.values()) | {k + 1 for k, x in enumerate(ins) if x.startswith(('s_branch', 's_cbranch'))} | {0})
    starts = [s for s in starts if s < len(ins)]
    nxt = dict(zip(starts, starts[1:] + [None]))
    def succ(s):
        e = (nxt[s] or len(ins)) - 1
        op, *arg = ins[e].split()
        if op == 's_endpgm': return []
        if op == 's_branch' or op == 's_cbranch_execnz': return [label_at[arg[0]]]
        if op.startswith('s_cbranch') and op != 's_cbranch_execz': return [label_at[arg[0]], nxt[s]]
        return [nxt[s]]
    return ins, label_at, nxt, succ


def trip_path(src, name, header, marker, steps, starts_too=False):
    """Instructions that a full trip issues from the loop header `header` (a block label) to the back edge: the body and
    the blocks behind it (the store, the flags, the loop control), which the per-label block above does not hold, without
    what the body's label holds but the trip does not run (the refill).  The function is cut into basic blocks at labels
    and branches; the path is the shortest one from the header back to it that issues `marker` at least `steps` times
    (leaving the loop and coming back in is shorter, but runs no step), taken with some lane live: s_cbranch_execz falls
    through and s_cbranch_execnz is taken, so the code under a lane mask counts.  Returns the count and the labels met."""
    import heapq
    ins, label_at, nxt, succ = cfg_of(src, name)
    size = lambda s: (nxt[s] or len(ins)) - s
    marks = lambda s: sum(1 for x in ins[s:s + size(s)] if x.split()[0] == marker)
    h = label_at[re.match(r'\.LBB\d+_\d+', header).group(0)]
    heap, seen = [(size(h), h, min(marks(h), steps), (h,))], set()
    while heap:
        cost, s, mk, path = heapq.heappop(heap)
        if (s, mk) in seen: continue
        seen.add((s, mk))
        for n in succ(s):
            if n is None: continue
            if n == h:
                if mk >= steps:
                    at = {v: k for k, v in label_at.items()}
                    return (cost, [at[p] for p in path if p in at]) + ((path,) if starts_too else ())
                continue
            heapq.heappush(heap, (cost + size(n), n, min(mk + marks(n), steps), path + (n,)))
    return (None, []) + (((),) if starts_too else ())


def refill_path(src, name, header, marker, steps):
    """Instructions that a 16-step trip issues on top of trip_path when it refills the ring: from behind the refill
    test's branch to the join behind the wave barrier.  The test is the one block of trip_path's route with a second
    way out that leaves the route and comes back to it further on; the figure is the shortest such detour, counted up to
    the block where it is back on the route.  Some lane is live on it (s_cbranch_execz falls through: code under a lane
    mask counts, which is the case of lanes of both parities crossing one quarter), and a scalar branch may take either
    way, so a second round that is skipped by a scalar test does not count while one that is only masked does."""
    import heapq
    ins, label_at, nxt, succ = cfg_of(src, name)
    n, _, route = trip_path(src, name, header, marker, steps, True)
    if n is None:
        return None
    size = lambda s: (nxt[s] or len(ins)) - s
    pos = {b: i for i, b in enumerate(route)}
    best = None
    for i, b in enumerate(route):
        for e in succ(b):
            if e is None or e in pos:
                continue
            heap, seen = [(0, e)], set()                 # (instructions issued before the block, the block)
            while heap:
                cost, s = heapq.heappop(heap)
                if s in seen: continue
                seen.add(s)
                if s in pos:
                    if pos[s] > i:                       # back on the route, further on: the join
                        best = cost if best is None else min(best, cost)
                        break
                    continue
                for m in succ(s):
                    if m is not None: heapq.heappush(heap, (cost + size(s), m))
    return best


def trip_tail(src, name, header, marker, steps):
    """Instructions that a 16-step trip issues, on the route a refilling trip takes, from the fence that closes the
    sixteenth issue_end (the body's last sched_barrier) to the wait in front of the next trip's first finish (the first
    s_waitcnt for lgkmcnt behind the loop header): what stands behind the body and in the loop header, where no read
    covers it.  It is trip_path, plus refill_path where the body itself holds no request (a global_load_dwordx4 in the
    body is the deferred refill: the detour that is left is the rare immediate one and does not count), less the
    instructions from that wait to that fence."""
    n, _ = trip_path(src, name, header, marker, steps)
    if n is None:
        return None
    i = src.index(name + ':')
    i = src.index(re.match(r'\.LBB\d+_\d+', header).group(0) + ':', i)
    k, first_wait, last_fence, marks, in_body_request = 0, None, None, 0, False
    for l in src[i:src.index('.Lfunc_end', i)].split('\n')[1:]:
        t = l.strip()
        if re.match(r'^\.LBB\d+_\d+:', l) and marks >= steps:
            break
        if t.startswith('; sched_barrier'):
            last_fence = k
        if not t or t.startswith(('.', ';')):
            continue
        op = t.split()[0]
        if op.startswith(('s_branch', 's_cbranch')) and marks >= steps:
            break
        if first_wait is None and op == 's_waitcnt' and 'lgkmcnt' in t:
            first_wait = k
        marks += op == marker
        in_body_request |= marks > 0 and op == 'global_load_dwordx4'
        k += 1
    if first_wait is None or last_fence is None:
        return None
    detour = 0 if in_body_request else (refill_path(src, name, header, marker, steps) or 0)
    return n + detour - (last_fence - first_wait)


GROUP_READ = ("ds_read_b128", r"ds_read_b32 .*offset:16\b")      # lookup_step_pk's group: 16 bytes + the dword after them
HEAD_READ = ("ds_read_b64", None)                                 # the head entry of the symbol just decoded


def to_json(out_path):
    """Instructions per step of the hot loop bodies (the largest block of each chain kernel that has no per-lane
    liveness selects, i.e. the body full trips take), keyed to the hash of the library built from the same sources:
    what bench.py's roofline.issue is computed from."""
    import glob, os, json, hashlib
    top = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    root = os.path.join(top, 'build', 'asm')
    with open(os.path.join(top, 'htscodecs_amd', 'librans4x16_hip.so'), 'rb') as f:
        sha = hashlib.sha256(f.read()).hexdigest()[:16]
    res = {"library_sha256_16": sha, "how": "make -C htscodecs_amd/csrc asm && python tools/isa_count.py --json <out>", "kernels": {}}
    for f in glob.glob(os.path.join(root, '*gfx950.s')):
        src = open(f).read()
        for name in sorted(set(re.findall(r'^(_Z\w+):', src, flags=re.M))):
            for pre, (label, marker, *least) in HOT.items():
                if not name.startswith(pre):
                    continue
                best, bodies = None, []
                for lab, b in blocks_of(src, name):
                    steps = sum(1 for x in b if x.split()[0] == marker)
                    if steps < (least[0] if least else 4):
                        continue
                    per = len(b) / steps
                    # every body of the kernel's loops (the encode chain has an affine and a look-up one: the latter reads idx_of[])
                    bodies.append({"steps_in_block": steps, "instructions_in_block": len(b), "instructions_per_step": round(per, 2),
                                   "ds_read_u8_in_block": sum(1 for x in b if x.split()[0] == "ds_read_u8")})
                    if best is None or per < best[0]:            # the leanest body with >= 4 steps: the full-trip one
                        c = Counter(x.split()[0] for x in b)
                        cat = lambda p: sum(v for k, v in c.items() if k.startswith(p))
                        best = (per, {"steps_in_block": steps, "instructions_per_step": round(per, 1),
                                      "valu_per_step": round(cat('v_') / steps, 1), "lds_per_step": round(cat('ds_') / steps, 1),
                                      "salu_and_waits_per_step": round(cat('s_') / steps, 1)})
                        if marker == "v_lshrrev_b64" and c["ds_read_b128"]:      # the decode chain on packed rows
                            best[1].update({"instructions_in_block": len(b), "s_waitcnt_in_block": c["s_waitcnt"],
                                            "s_nop_in_block": c["s_nop"],
                                            "group_shadow_per_step": shadows(b, *GROUP_READ),
                                            "head_shadow_per_step": shadows(b, *HEAD_READ)})
                            if least:                                    # the 16-step trip: header to back edge, no refill
                                n, labs = trip_path(src, name, lab, marker, least[0])
                                best[1].update({"trip_path_instructions": n, "trip_path_blocks": labs,
                                                "refill_path_instructions": refill_path(src, name, lab, marker, least[0]),
                                                "trip_tail_instructions": trip_tail(src, name, lab, marker, least[0])})
                if best:
                    res["kernels"][label] = best[1]
                    res["kernels"][label]["bodies"] = bodies
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def main():
    import glob, os
    if len(sys.argv) > 2 and sys.argv[1] == '--json':
        return to_json(sys.argv[2])
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'build', 'asm')
    want = sys.argv[1]
    sub = sys.argv[2] if len(sys.argv) > 2 else ''
    for f in glob.glob(os.path.join(root, '*gfx950.s')):
        src = open(f).read()
        for name in sorted(set(re.findall(r'^(_Z\w+):', src, flags=re.M))):
            if want not in name:
                continue
            bl = [b for b in blocks_of(src, name) if sub in b[0]]
            for lab, b in sorted(bl, key=lambda b: -len(b[1]))[:2]:
                c = Counter(x.split()[0] for x in b)
                cat = lambda p: sum(v for k, v in c.items() if k.startswith(p))
                print(f"{name}\n  {lab[:100]}\n  total {len(b)}  valu {cat('v_')}  ds {cat('ds_')}  salu {cat('s_')}  vmem {cat('global_') + cat('buffer_') + cat('flat_')}")
                print('  ', c.most_common(50))
                if c["ds_read_b128"]:
                    print('   group shadow per step', shadows(b, *GROUP_READ), ' head shadow per step', shadows(b, *HEAD_READ))
                    steps = c["ds_read_b128"]
                    if steps >= 16:
                        print('   trip path, header to back edge without the refill', trip_path(src, name, lab, "v_lshrrev_b64", steps))
                        print('   refill path, behind the test to the join', refill_path(src, name, lab, "v_lshrrev_b64", steps))
                        print('   trip tail, the last fence to the first wait on the refilling route', trip_tail(src, name, lab, "v_lshrrev_b64", steps))

if __name__ == '__main__':
    main()
