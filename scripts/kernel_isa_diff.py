"""Kernel ISA diff of two source trees (manual tool, not a test; needs no GPU): proves that a change of the HIP sources - a helper moved
into a shared header, a block turned into a function - left every kernel's machine code as it was.

For each named .hip file of chameleon_recsys_amd/csrc the tool compiles the file of both trees to gfx950 assembly (build.FLAGS of THIS
tree plus --cuda-device-only -S, every translation unit in a process of its own), cuts the assembly by kernel symbol into the kernel's body
and its .amdhsa_kernel descriptor block (registers, LDS, scratch), drops the comment lines and compares the text.  Local labels carry the
position of their function in the file (.LBB<function>_<block>): that index is dropped, so a kernel that is merely emitted earlier or later
still compares equal.  Nothing else is looked at.
  python scripts/kernel_isa_diff.py OLD_TREE NEW_TREE [--files a.hip b.hip ...] [--keep DIR]
prints one line per kernel - same | differs | added | removed - and exits non-zero unless every kernel is `same`."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chameleon_recsys_amd import build  # noqa: E402

DEFAULT_FILES = ["gemm.hip", "gemm_x3.hip", "gemm_b16.hip", "gemm_p3.hip", "gemm_h2.hip", "dm_fused.hip"]
CSRC = os.path.join("chameleon_recsys_amd", "csrc")


def compile_asm(tree, files, out_dir):
    """{file: path of its assembly}; the translation units of one tree compile in parallel."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    procs = []
    for f in files:
        out = os.path.join(out_dir, f.replace(".hip", ".s"))
        cmd = [hipcc] + build.FLAGS + ["--cuda-device-only", "-S", os.path.join(tree, CSRC, f), "-o", out]
        procs.append((f, out, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    asm = {}
    for f, out, p in procs:
        log, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(log.decode())
            raise RuntimeError("hipcc failed on %s of %s" % (f, tree))
        asm[f] = out
    return asm


def kernels(path):
    """{kernel symbol: (body lines, descriptor lines)} of one assembly file."""
    with open(path) as fh:
        lines = [ln.split(";", 1)[0].rstrip() for ln in fh]                    # comment lines, trailing comments
    lines = [re.sub(r"\.L([A-Za-z_]+)\d+_(\d+)", r".L\1_\2", ln) for ln in lines]   # .LBB12_3 -> .LBB_3
    lines = [ln for ln in lines if ln.strip()]
    out = {ln.split()[1]: ([], []) for ln in lines if ln.lstrip().startswith(".amdhsa_kernel ")}
    body = desc = None
    for ln in lines:
        if desc is not None:                                                   # .amdhsa_kernel NAME ... .end_amdhsa_kernel
            if ln.lstrip().startswith(".end_amdhsa_kernel"):
                desc = None
            else:
                desc.append(ln)
        elif body is not None:                                                 # NAME: ... .Lfunc_endN: (a kernel may hold more than one s_endpgm)
            if ln.startswith(".Lfunc_end"):
                body = None
            else:
                body.append(ln)
        elif ln.endswith(":") and ln[:-1] in out:
            body = out[ln[:-1]][0]
        elif ln.lstrip().startswith(".amdhsa_kernel "):
            desc = out[ln.split()[1]][1]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--files", nargs="+", default=DEFAULT_FILES)
    ap.add_argument("--keep", default=None, help="keep the assembly files in DIR/old and DIR/new")
    args = ap.parse_args()
    tmp = args.keep or tempfile.mkdtemp(prefix="kernel_isa_diff_")
    dirs = {}
    for tag in ("old", "new"):
        dirs[tag] = os.path.join(tmp, tag)
        os.makedirs(dirs[tag], exist_ok=True)
    old = compile_asm(args.old_tree, args.files, dirs["old"])
    new = compile_asm(args.new_tree, args.files, dirs["new"])
    counts = {"same": 0, "differs": 0, "added": 0, "removed": 0}
    for f in args.files:
        ko, kn = kernels(old[f]), kernels(new[f])
        for name in sorted(set(ko) | set(kn)):
            if name not in kn:
                verdict = "removed"
            elif name not in ko:
                verdict = "added"
            elif ko[name] == kn[name]:
                verdict = "same"
            else:
                verdict = "differs (%s)" % ("body" if ko[name][0] != kn[name][0] else "descriptor")
            counts[verdict.split()[0]] += 1
            print("%-14s %-18s %s  [%d lines]" % (f, verdict, name, len((kn.get(name) or ko[name])[0])))
    print("kernels: %(same)d same, %(differs)d differs, %(added)d added, %(removed)d removed" % counts)
    return 0 if counts["same"] and not (counts["differs"] or counts["added"] or counts["removed"]) else 1


if __name__ == "__main__":
    sys.exit(main())
