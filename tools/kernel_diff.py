#!/usr/bin/env python
"""Did moving code between translation units change a kernel?  Compares the compiler's output, kernel by kernel.

    tools/kernel_diff.py --rev HEAD~1 --old ptmi_abi.hip --new ptmi_abi.hip ptmi_cov.hip ptmi_am_ahead.hip

compiles the --old units of csrc/ as they are at the git revision --rev and the --new units of the working tree, each with the
library's own flags (_build.FLAGS) plus --cuda-device-only -S, and compares for every kernel
  * its instructions: the assembly from the kernel's label to its .Lfunc_end, with the local labels that carry the function's
    number in the unit renamed (.LBB<n>_ -> .LBB_, likewise .Ltmp, .Lfunc_*, .LJTI, and the long branches' .Lpost_getpc<n>, which
    are numbered through the unit), comments and blank lines dropped;
  * its .amdhsa_kernel ... .end_amdhsa_kernel block: registers, scratch, LDS and every other field of the descriptor.
A shape unit (ptmi_shape.hip) is compiled with -D defines and scheduler options of its own:

    tools/kernel_diff.py --rev HEAD~1 --old ptmi_shape.hip --new ptmi_shape.hip --defs 4,5,2,0

takes them from _build.shape_defs(G, E, family, part); --defs "-DNAME=1 ..." passes a literal list to both sides instead.
--rename PATTERN REPLACEMENT (a regular expression, may repeat) rewrites the OLD side's assembly before it is compared, for a
change that only alters how a kernel's name is mangled, such as a template parameter added with a default.
It prints the number of kernels on each side, the names that are missing, extra or defined twice, and the kernels whose text
or descriptor differs; the exit status is 0 only when there is none of those.  Needs hipcc, no GPU."""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ptmcmcsampler_amd import _build  # noqa: E402

CSRC = os.path.relpath(_build.CSRC, ROOT)
LOCAL = [(re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Ltmp\d+"), ".Ltmp"), (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1"),
         (re.compile(r"\.LJTI\d+_"), ".LJTI_"), (re.compile(r"\.Lpost_getpc\d+"), ".Lpost_getpc")]


DEFS = []       # --defs: the unit's own defines and options, for both sides


def assembly(src, out):
    subprocess.run([_build.hipcc()] + _build.FLAGS + DEFS + ["--cuda-device-only", "-S", src, "-o", out], check=True)
    return open(out).read()


def unit_defs(text):
    """--defs G,E,FAMILY,PART -> _build.shape_defs of that shape unit; anything else is a literal list of compiler arguments."""
    if re.fullmatch(r"\d+,\d+,\d+,\d+", text.strip()):
        return _build.shape_defs(*[int(v) for v in text.split(",")])
    return text.split()


def clean(lines):
    """Comments and blank lines dropped, the function-numbered local labels renamed."""
    res = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip():
            continue
        for pat, to in LOCAL:
            ln = pat.sub(to, ln)
        res.append(ln)
    return res


def kernels(asm):
    """{name: (instruction text, descriptor block)} of one unit's assembly; a kernel is what has an .amdhsa_kernel block."""
    lines = asm.split("\n")
    desc = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            desc[m.group(1)] = clean(lines[i:end + 1])
    res = {}
    for name, block in desc.items():
        i = next(j for j, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(j for j in range(i, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[j]))
        res[name] = (clean(lines[i:end + 1]), block)
    return res


def side(label, paths, tmp, jobs, rename=()):
    """The kernels of a set of units, and the names defined in more than one of them."""
    outs = [os.path.join(tmp, "%s_%d.s" % (label, i)) for i in range(len(paths))]
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        asms = list(pool.map(assembly, paths, outs))
    for pat, to in rename:
        asms = [re.sub(pat, to, asm) for asm in asms]
    found, twice = {}, []
    for path, asm in zip(paths, asms):
        ks = kernels(asm)
        print("%s  %-24s %3d kernels" % (label, os.path.basename(path), len(ks)))
        for name, k in ks.items():
            if name in found:
                twice.append(name)
            found[name] = k
    return found, twice


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rev", default="HEAD", help="git revision the --old units are taken from [HEAD]")
    ap.add_argument("--old", nargs="+", required=True, metavar="UNIT", help="units of csrc/ at --rev")
    ap.add_argument("--new", nargs="+", required=True, metavar="UNIT", help="units of csrc/ in the working tree")
    ap.add_argument("--jobs", type=int, default=min(8, _build._usable_cores()))
    ap.add_argument("--defs", default="", metavar="G,E,FAMILY,PART | ARGS", help="a shape unit's defines and options (_build.shape_defs), or a literal list")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("PATTERN", "REPLACEMENT"),
                    help="re.sub over the old side's assembly before the comparison (may repeat)")
    a = ap.parse_args()
    DEFS[:] = unit_defs(a.defs)
    with tempfile.TemporaryDirectory() as tmp:
        # the revision's csrc/ and include/ side by side, as the units' #include lines expect them
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.rev, CSRC, "include"], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        old, old_twice = side("old", [os.path.join(tmp, CSRC, u) for u in a.old], tmp, a.jobs, a.rename)
        new, new_twice = side("new", [os.path.join(ROOT, CSRC, u) for u in a.new], tmp, a.jobs)
    missing, extra = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    text = sorted(k for k in set(old) & set(new) if old[k][0] != new[k][0])
    desc = sorted(k for k in set(old) & set(new) if old[k][1] != new[k][1])
    print("kernels: %d old (%s), %d new" % (len(old), a.rev, len(new)))
    for what, names in (("missing from new", missing), ("extra in new", extra), ("defined twice in old", old_twice), ("defined twice in new", new_twice),
                        ("instruction text differs", text), (".amdhsa_kernel block differs", desc)):
        print("%-30s %d%s" % (what + ":", len(names), "".join("\n    " + n for n in names)))
    return 1 if missing or extra or old_twice or new_twice or text or desc else 0


if __name__ == "__main__":
    sys.exit(main())
