"""Instruction mix of a kernel, inside and outside its MFMA chains: python tools/isa_mix.py file.s kernel_substring [--top N] [--gap G] [--loop]
Input: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include -S --cuda-device-only csrc/split.hip (host only; as tools/isa_spills.py).
Counts instructions by class (MFMA, vector, LDS, vector memory, scalar, s_waitcnt, s_nop).  A chain is the span from the first to the
last MFMA of a run of MFMAs; a run ends where more than G (default 40) other instructions follow an MFMA.  What lies outside the chains is
what both waves of a SIMD pay in full (docs/experiments.md), so the most frequent vector mnemonics out there are listed.
--loop: only the tile loop (the backward branch that spans the most MFMAs).  Also importable: kernel_body, tile_loop, mix, resources."""
import collections
import re
import sys

CLASSES = ("mfma", "vector", "lds", "vmem", "scalar", "s_waitcnt", "s_nop")


def kernel_body(lines, key):
    """(start, end) line numbers of the first function whose mangled name contains key"""
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and ":" in l and key in l.split(":")[0])
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return start, end


def instructions(lines, start, end):
    """[(line number, mnemonic, operand text)] of the instructions between two lines; labels as (n, 'label', name)"""
    out = []
    for i in range(start + 1, end):
        l = lines[i].split(";")[0].strip()
        if not l:
            continue
        if l.endswith(":"):
            out.append((i, "label", l[:-1]))
        elif not l.startswith("."):
            m, _, ops = l.partition(" ")
            out.append((i, m, ops.strip()))
    return out


def tile_loop(ins):
    """the slice of ins between a label and the backward branch to it that spans the most MFMAs"""
    where = {name: k for k, (_, m, name) in enumerate(ins) if m == "label"}
    best = (0, 0, len(ins))
    for k, (_, m, ops) in enumerate(ins):
        if m.startswith("s_cbranch") or m == "s_branch":
            t = where.get(ops.split()[-1])
            if t is not None and t < k:
                n = sum(1 for x in ins[t:k] if x[1].startswith("v_mfma"))
                if n > best[0]:
                    best = (n, t, k + 1)
    return ins[best[1]:best[2]]


def classify(m):
    if m.startswith("v_mfma") or m.startswith("v_smfmac"): return "mfma"
    if m.startswith("ds_"): return "lds"
    if m.startswith(("global_", "buffer_", "flat_", "scratch_")): return "vmem"
    if m == "s_waitcnt": return "s_waitcnt"
    if m == "s_nop": return "s_nop"
    if m.startswith("v_"): return "vector"
    if m.startswith("s_"): return "scalar"
    return None


def mix(ins, gap=40):
    """({class: count} inside chains, the same outside, Counter of vector mnemonics outside, number of chains)"""
    real = [(m, ops) for _, m, ops in ins if m != "label" and classify(m)]
    inside = [False] * len(real)
    pos = [k for k, (m, _) in enumerate(real) if classify(m) == "mfma"]
    chains = 0
    k = 0
    while k < len(pos):
        j = k
        while j + 1 < len(pos) and pos[j + 1] - pos[j] - 1 <= gap:
            j += 1
        for q in range(pos[k], pos[j] + 1):
            inside[q] = True
        chains += 1
        k = j + 1
    cin, cout, vout = collections.Counter(), collections.Counter(), collections.Counter()
    for (m, _), ins_ in zip(real, inside):
        (cin if ins_ else cout)[classify(m)] += 1
        if not ins_ and classify(m) == "vector":
            vout[re.sub(r"_e(32|64)$|_dpp$|_sdwa$", "", m)] += 1
    return cin, cout, vout, chains


def resources(lines, key):
    """the kernel's resource lines of the metadata (vgpr, agpr, sgpr counts, spills, scratch size)"""
    out = {}
    for i, l in enumerate(lines):
        if ".name:" in l and key in l:
            for j in range(max(0, i - 14), min(len(lines), i + 14)):
                m = re.match(r"\s*\.(vgpr_count|agpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s*(\d+)", lines[j])
                if m:
                    out[m.group(1)] = int(m.group(2))
            break
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = {sys.argv[i]: sys.argv[i + 1] for i in range(1, len(sys.argv) - 1) if sys.argv[i] in ("--top", "--gap")}
    for v in opt.values():
        args.remove(v)
    src, key = args
    lines = open(src).read().splitlines()
    s, e = kernel_body(lines, key)
    ins = instructions(lines, s, e)
    if "--loop" in sys.argv:
        ins = tile_loop(ins)
    cin, cout, vout, chains = mix(ins, int(opt.get("--gap", 40)))
    print(f"{lines[s].split(':')[0]}{'  (tile loop)' if '--loop' in sys.argv else ''}: {chains} chains")
    print(f"{'class':10s} {'in chain':>9s} {'outside':>9s}")
    for c in CLASSES:
        print(f"{c:10s} {cin[c]:9d} {cout[c]:9d}")
    print("vector instructions outside chains:")
    for m, n in vout.most_common(int(opt.get("--top", 12))):
        print(f"  {n:5d}  {m}")
    print("  ".join(f"{k} {v}" for k, v in resources(lines, key).items()))
