"""LDS waits of a kernel's MFMA chains: python tools/isa_chain.py file.s kernel_substring [--gap G] [--all]
Input and chain definition: as tools/isa_mix.py (host only; the tile loop of the kernel, --all: the whole kernel).
Per chain it prints
  * the forms of its s_waitcnt instructions (how many drain the LDS queue, lgkmcnt(0), and how many wait for a count);
  * for the fragment reads (ds_read_b128): how far ahead of the wait that covers them they are issued -- MFMAs and other instructions
    between the read and the first s_waitcnt that retires it, as (minimum, median, maximum) and as a histogram over the MFMA distance.
The LDS queue is retired in order, so a read issued with k younger LDS instructions behind it is covered by the first wait whose
lgkmcnt is at most k.  Scalar memory loads share the counter and return out of order; hipcc drains (lgkmcnt(0)) where one is pending, and
a drain covers everything, so they are not modelled."""
import collections
import re
import sys

import isa_mix


def chains(ins, gap=40):
    """[(first, last)] index ranges into ins (labels dropped by the caller) of the MFMA chains, as isa_mix.mix delimits them"""
    pos = [k for k, (_, m, _) in enumerate(ins) if isa_mix.classify(m) == "mfma"]
    out, k = [], 0
    while k < len(pos):
        j = k
        while j + 1 < len(pos) and pos[j + 1] - pos[j] - 1 <= gap:
            j += 1
        out.append((pos[k], pos[j]))
        k = j + 1
    return out


def lgkm(ops):
    """the lgkmcnt of an s_waitcnt's operand text, None if it does not wait on that counter"""
    m = re.search(r"lgkmcnt\((\d+)\)", ops)
    return int(m.group(1)) if m else None


def chain_report(ins, first, last):
    forms = collections.Counter()
    pending = []                     # LDS instructions in flight, oldest first: [index into ins, is fragment read]
    dist = []                        # (MFMAs, other instructions) between a fragment read and the wait that covers it
    uncovered = 0
    for k in range(first, last + 1):
        _, m, ops = ins[k]
        if m == "s_waitcnt":
            forms[re.sub(r"\s+", " ", ops)] += 1
            n = lgkm(ops)
            if n is not None:
                while len(pending) > n:
                    at, frag = pending.pop(0)
                    if frag:
                        between = [isa_mix.classify(x[1]) for x in ins[at + 1:k]]
                        nm = sum(1 for c in between if c == "mfma")
                        dist.append((nm, len(between) - nm))
        elif isa_mix.classify(m) == "lds":
            pending.append([k, m.startswith("ds_read_b128")])
    uncovered = sum(1 for _, frag in pending if frag)
    return forms, dist, uncovered


def med(v):
    v = sorted(v)
    return v[len(v) // 2] if v else 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    gap = 40
    if "--gap" in sys.argv:
        g = sys.argv[sys.argv.index("--gap") + 1]
        gap = int(g)
        args.remove(g)
    src, key = args
    lines = open(src).read().splitlines()
    s, e = isa_mix.kernel_body(lines, key)
    ins = isa_mix.instructions(lines, s, e)
    if "--all" not in sys.argv:
        ins = isa_mix.tile_loop(ins)
    ins = [x for x in ins if x[1] != "label" and isa_mix.classify(x[1])]
    print(f"{lines[s].split(':')[0]}{'' if '--all' in sys.argv else '  (tile loop)'}")
    for c, (a, b) in enumerate(chains(ins, gap)):
        forms, dist, unc = chain_report(ins, a, b)
        nm = sum(1 for x in ins[a:b + 1] if isa_mix.classify(x[1]) == "mfma")
        drains = sum(n for f, n in forms.items() if lgkm(f) == 0)
        counted = sum(n for f, n in forms.items() if (lgkm(f) or 0) > 0)
        print(f"chain {c}: {nm} MFMAs, {sum(forms.values())} s_waitcnt: {drains} lgkmcnt(0), {counted} lgkmcnt(n > 0), {sum(forms.values()) - drains - counted} other")
        print("   forms: " + "  ".join(f"{n} x {f}" for f, n in forms.most_common()))
        if dist:
            dm, do = [d[0] for d in dist], [d[1] for d in dist]
            hist = collections.Counter(dm)
            print(f"   fragment ds_read_b128: {len(dist)} covered inside the chain ({unc} by a wait behind it); MFMAs between read and wait min {min(dm)} "
                  f"median {med(dm)} max {max(dm)}; other instructions min {min(do)} median {med(do)} max {max(do)}")
            print("   reads by MFMA distance: " + "  ".join(f"{d}: {hist[d]}" for d in sorted(hist)))
