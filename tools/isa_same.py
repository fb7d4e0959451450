#!/usr/bin/env python3
"""Do two checkouts compile to the same gfx950 kernels?  The acceptance test of a refactor of plslam_amd/csrc.

usage: isa_same.py <checkout or csrc dir A> <checkout or csrc dir B> [source.hip ...]

Compiles every source of the product and of the legacy build (or the sources named) in both trees to device assembly with
the flags plslam_amd/build.py gives that source, splits the listing per function symbol and compares, symbol by symbol, the
instruction stream with its .amdhsa_ block and the kernel's entry in the code-object metadata (VGPRs, AGPRs, SGPRs, LDS
and scratch bytes, spill counts, arguments); what is outside every function (LDS and constant symbols) is compared as
"<file scope>".  Normalised away: comments, .file / .loc / .ident lines, the numbering of local labels and the
__hip_cuid_<hash> symbol (derived from the file's text); nothing else.  Needs no GPU.  Exit status 1 when anything differs."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plslam_amd import build as B  # noqa: E402


def tree(path):
    """(csrc, include) of a checkout, or of a bare csrc directory (then the include directory two levels up, else ours)."""
    path = os.path.abspath(path)
    csrc = path if os.path.exists(os.path.join(path, "common.hpp")) else os.path.join(path, "plslam_amd", "csrc")
    inc = os.path.join(os.path.dirname(os.path.dirname(csrc)), "include")
    return csrc, inc if os.path.isdir(inc) else os.path.join(B._ROOT, "include")


def assembly(t, src, legacy):
    csrc, inc = t
    flags = [f.replace(B.CSRC, csrc) for f in B._flags_for(src, legacy) if not f.startswith("-I")] + ["-I" + inc]
    r = subprocess.run([B.hipcc_path()] + flags + ["-S", "--cuda-device-only", os.path.join(csrc, src), "-o", "-"],
                       capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"hipcc failed on {os.path.join(csrc, src)}:\n{r.stderr[-3000:]}")
    return r.stdout


def normal(lines):
    out, labels = [], {}
    for l in lines:
        l = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", l.split(";")[0].rstrip())
        if l.strip() and not re.match(r"\s*\.(file|loc|ident)\b", l):
            out.append(re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), l))
    return out


def split(text):
    """{symbol: {"code": [...], "metadata": [...]}} of one listing."""
    body, _, meta = text.partition("\t.amdgpu_metadata")
    parts, name, cur, rest = {}, None, [], []
    for l in body.split("\n"):
        m = re.match(r"\s*\.type\s+([\w.$]+),@function", l)
        if m:
            name, cur = m.group(1), []
        (rest if name is None else cur).append(l)
        if name is not None and re.match(r"\.Lfunc_end\d+:", l):
            parts[name], name = {"code": normal(cur), "metadata": []}, None
    parts["<file scope>"] = {"code": normal(rest), "metadata": []}
    for entry in re.split(r"^  - (?=\.agpr_count:)", meta, flags=re.M)[1:]:
        entry = entry.split("\namdhsa.")[0]
        parts.setdefault(re.search(r"\.name:\s+(\S+)", entry).group(1), {"code": []})["metadata"] = normal(entry.split("\n"))
    return parts


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, b = tree(sys.argv[1]), tree(sys.argv[2])
    jobs = [(s, False) for s in B.SOURCES] + [(s, True) for s in B.LEGACY_SOURCES + list(B.LEGACY_AWARE)]
    if sys.argv[3:]:
        jobs = [j for j in jobs if j[0] in sys.argv[3:]]
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 2))) as ex:
        listings = list(ex.map(lambda j: (split(assembly(a, *j)), split(assembly(b, *j))), jobs))
    total, differing = 0, []
    for (src, legacy), (pa, pb) in zip(jobs, listings):
        bad = []
        for sym in sorted(set(pa) | set(pb)):
            if sym not in pa or sym not in pb:
                bad.append(f"    {sym}: only in {'B' if sym in pb else 'A'}")
            elif pa[sym] != pb[sym]:
                bad.append(f"    {sym}: {', '.join(k for k in ('code', 'metadata') if pa[sym][k] != pb[sym][k])} differs")
        kernels = sum(1 for v in pb.values() if v["metadata"])
        total += kernels
        print(f"{src:22s} {'legacy ' if legacy else 'product'}  {kernels:3d} kernels, {len(pb) - 1:3d} symbols: "
              + ("identical" if not bad else f"{len(bad)} DIFFER"))
        print("\n".join(bad), end="\n" if bad else "")
        differing += [(src, l) for l in bad]
    print(f"{len(jobs)} compilations, {total} kernels: " + ("all identical" if not differing else f"{len(differing)} symbols differ"))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
