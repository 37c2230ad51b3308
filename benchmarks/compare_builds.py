#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, kernel by kernel.

    python3 benchmarks/compare_builds.py PARENT BRANCH

PARENT and BRANCH are two `.s` files, or two directories of them, as written by
`hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S` (or --save-temps).  Per kernel: present in both or not, the
resource directives of its .amdhsa_kernel block, from them the allocated VGPRs (granule of 8) and the waves per SIMD of a 512-register
file, and whether the instruction text is equal once labels are renumbered and comments, .loc and blank lines are dropped.  It compares
two texts; it knows nothing about what the instructions are.  The exit status is 1 when a kernel is missing on one side, gains LDS or
scratch, or loses a wave per SIMD -- the bar the refactor records under profiles/ were held to."""
import os
import re
import sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def kernels(path):
    """{kernel name: (normalised text, {directive: value})} of one .s file"""
    lines = open(path, errors="replace").read().split("\n")
    res, out = {}, {}
    name = None
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            name = m.group(1)
            res[name] = {}
        elif name and ".end_amdhsa_kernel" in ln:
            name = None
        elif name:
            m = re.match(r"\s*\.amdhsa_(\w+)\s+(\d+)", ln)
            if m and m.group(1) in FIELDS:
                res[name][m.group(1)] = int(m.group(2))
    for name in res:
        try:
            i = next(k for k, ln in enumerate(lines) if ln.startswith(name + ":"))
        except StopIteration:
            continue
        body, seen = [], {}
        for ln in lines[i + 1:]:
            if re.match(r"\.Lfunc_end\d+:", ln):
                break
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith((".loc", ".file", ".cfi_", ".p2align")):
                continue
            body.append(LABEL.sub(lambda m: seen.setdefault(m.group(0), "L%d" % len(seen)), ln))
        out[name] = ("\n".join(body), res[name])
    return out


def files(path):
    if os.path.isdir(path):
        return {f: os.path.join(path, f) for f in sorted(os.listdir(path)) if f.endswith(".s")}
    return {os.path.basename(path): path}


def occupancy(r):
    alloc = -(-r.get("next_free_vgpr", 0) // 8) * 8
    return alloc, min(8, 512 // alloc) if alloc else 8


def short(name):
    try:
        import subprocess
        full = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    except OSError:
        return name
    full = full.replace("(anonymous namespace)::", "")
    return re.sub(r"^void ", "", full).split("(")[0] or name


def main(a, b):
    fa, fb = files(a), files(b)
    if len(fa) == 1 and len(fb) == 1:
        fb = {next(iter(fa)): next(iter(fb.values()))}
    bad = 0
    for f in sorted(set(fa) | set(fb)):
        if f not in fa or f not in fb:
            print("%s: only in %s" % (f, a if f in fa else b))
            bad += 1
            continue
        ka, kb = kernels(fa[f]), kernels(fb[f])
        equal = 0
        for name in sorted(set(ka) | set(kb)):
            if name not in ka or name not in kb:
                print("  %s: only in the %s build" % (short(name), "first" if name in ka else "second"))
                bad += 1
                continue
            (ta, ra), (tb, rb) = ka[name], kb[name]
            (alloc_a, wa), (alloc_b, wb) = occupancy(ra), occupancy(rb)
            worse = [k for k in FIELDS[3:] if rb.get(k, 0) > ra.get(k, 0)] + (["waves"] if wb < wa else [])
            bad += bool(worse)
            if ta == tb and ra == rb:
                equal += 1
                continue
            print("  %s: text %s%s" % (short(name), "equal" if ta == tb else "differs", "  WORSE: " + ", ".join(worse) if worse else ""))
            for tag, r, alloc, w in (("first ", ra, alloc_a, wa), ("second", rb, alloc_b, wb)):
                print("    %s %s  vgpr alloc %d  waves/SIMD %d" % (tag, "  ".join("%s %d" % (k, r.get(k, 0)) for k in FIELDS), alloc, w))
        print("%s: %d kernels / %d, same names: %s, text and resources equal: %d" % (
            f, len(ka), len(kb), "yes" if set(ka) == set(kb) else "NO", equal))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
