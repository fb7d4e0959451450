#!/usr/bin/env python3
"""Do two checkouts compile to the same gfx950 kernels?  The acceptance test of a refactor of plslam_amd/csrc.

usage: isa_same.py <checkout or csrc dir A> <checkout or csrc dir B> [source.hip ...]

Compiles every source of the product and of the legacy build (or the sources named) in both trees to device assembly with
the flags plslam_amd/build.py gives that source, splits the listing per function symbol and compares, symbol by symbol, the
instruction stream with its .amdhsa_ block and the kernel's entry in the code-object metadata (VGPRs, AGPRs, SGPRs, LDS
and scratch bytes, spill counts, arguments); what is outside every function (LDS and constant symbols) is compared as
"<file scope>".  Each tree is compiled from its own plslam_amd/build.py (source lists and flags).  A source both trees have is
compared file against file (unless its functions are not the same set in both: it was split or merged); then the function symbols of the whole product library, and of the whole legacy library, are
compared by name, so a kernel that moved to another file is matched and "only in A / B" is said of the library.  The file
scope of the sources only one tree has is compared as the set of its lines.  Normalised away: comments, .file / .loc / .ident lines, the numbering of local labels and the
__hip_cuid_<hash> symbol (derived from the file's text); nothing else.  Needs no GPU.  Exit status 1 when anything differs."""
import importlib.util
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plslam_amd import build as B  # noqa: E402


def tree(path):
    """(csrc, include, build module) of a checkout, or of a bare csrc directory (then the include directory two levels up and
    the build.py beside it, else ours)."""
    path = os.path.abspath(path)
    csrc = path if os.path.exists(os.path.join(path, "common.hpp")) else os.path.join(path, "plslam_amd", "csrc")
    inc = os.path.join(os.path.dirname(os.path.dirname(csrc)), "include")
    build, Bt = os.path.join(os.path.dirname(csrc), "build.py"), B
    if os.path.exists(build) and not os.path.samefile(build, B.__file__):
        spec = importlib.util.spec_from_file_location("build_of_" + re.sub(r"\W", "_", path), build)
        Bt = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(Bt)
    return csrc, inc if os.path.isdir(inc) else os.path.join(B._ROOT, "include"), Bt


def jobs_of(t):
    Bt = t[2]
    return [(s, False) for s in Bt.SOURCES] + [(s, True) for s in Bt.LEGACY_SOURCES + list(Bt.LEGACY_AWARE)]


def assembly(t, src, legacy):
    csrc, inc, Bt = t
    flags = [f.replace(Bt.CSRC, csrc) for f in Bt._flags_for(src, legacy) if not f.startswith("-I")] + ["-I" + inc]
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


def library(t, listing, legacy, shared):
    """{symbol: [its bodies, sorted]} over the sources of one library of tree t; "<file scope>": the set of file-scope lines of
    its sources outside `shared` (the shared ones are compared file against file), local labels without their numbers."""
    Bt, syms, scope = t[2], {}, set()
    for src in Bt.SOURCES + (Bt.LEGACY_SOURCES if legacy else []):
        for sym, v in listing[(src, legacy and (src, True) in listing)].items():
            if sym != "<file scope>":
                syms.setdefault(sym, []).append(v)
            elif src not in shared:
                scope |= {re.sub(r"\.L\d+", ".L", l) for l in v["code"]}
    return {**{k: sorted(v, key=repr) for k, v in syms.items()}, "<file scope>": sorted(scope)}


def differences(pa, pb):
    bad = []
    for sym in sorted(set(pa) | set(pb)):
        if sym not in pa or sym not in pb:
            bad.append(f"    {sym}: only in {'B' if sym in pb else 'A'}")
        elif pa[sym] != pb[sym]:
            bad.append(f"    {sym}: differs" if isinstance(pa[sym], list) else
                       f"    {sym}: {', '.join(k for k in ('code', 'metadata') if pa[sym][k] != pb[sym][k])} differs")
    return bad


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, b = tree(sys.argv[1]), tree(sys.argv[2])
    ja, jb = jobs_of(a), jobs_of(b)
    if sys.argv[3:]:
        ja, jb = ([j for j in jobs if j[0] in sys.argv[3:]] for jobs in (ja, jb))
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 2))) as ex:
        la, lb = (dict(zip(jobs, ex.map(lambda j: split(assembly(t, *j)), jobs))) for t, jobs in ((a, ja), (b, jb)))
    total, differing = 0, []

    def report(title, kernels, symbols, bad):
        print(f"{title}  {kernels:3d} kernels, {symbols:3d} symbols: " + ("identical" if not bad else f"{len(bad)} DIFFER"))
        print("\n".join(bad), end="\n" if bad else "")
        differing.extend((title, l) for l in bad)

    # a source both trees have whose functions are not the same set was split or merged: library-wide, like a new source
    moved = {j for j in jb if j in la and set(la[j]) != set(lb[j])}
    for src, legacy in [j for j in jb if j in la]:
        pa, pb = la[(src, legacy)], lb[(src, legacy)]
        kernels = sum(1 for v in pb.values() if v["metadata"])
        total += kernels
        if (src, legacy) in moved:
            print(f"{src:22s} {'legacy ' if legacy else 'product'}  {kernels:3d} kernels: other functions than in A, compared library-wide")
            continue
        report(f"{src:22s} {'legacy ' if legacy else 'product'}", kernels, len(pb) - 1, differences(pa, pb))
    for side, mine, other in (("A", la, lb), ("B", lb, la)):
        for src, legacy in [j for j in mine if j not in other]:
            kernels = sum(1 for v in mine[(src, legacy)].values() if v["metadata"])
            total += kernels if side == "B" else 0
            print(f"{src:22s} {'legacy ' if legacy else 'product'}  {kernels:3d} kernels: only in {side}, compared library-wide")
    if not sys.argv[3:]:
        shared = ({j[0] for j in ja} & {j[0] for j in jb}) - {j[0] for j in moved}
        for legacy in (False, True):
            ua, ub = library(a, la, legacy, shared), library(b, lb, legacy, shared)
            kernels = sum(1 for sym, bodies in ub.items() if sym != "<file scope>" and any(v["metadata"] for v in bodies))
            report(f"{'every source, by symbol':22s} {'legacy ' if legacy else 'product'}", kernels, len(ub) - 1, differences(ua, ub))
    print(f"{len(ja)} + {len(jb)} compilations, {total} kernels: " + ("all identical" if not differing else f"{len(differing)} symbols differ"))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
