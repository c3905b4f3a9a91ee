#!/usr/bin/env python3
"""Kernel count and SHA-256 of the gfx950 device assembly of a .hip file, compiled with the product flags:
    tools/isa_digest.py jpeg_amd/csrc/kernels_quad.hip [-DMACRO ...]
Equal digests before and after a refactor mean the same instructions, registers and LDS: no kernel changed.  The lines that
contain __hip_cuid_ are left out (that symbol hashes the source text); nothing else of the assembly is looked at.
    tools/isa_digest.py --kernels FILE [-DMACRO ...]
One line per kernel instead: the demangled name, the number of instructions and a SHA-256 of the instruction lines, for a
refactor after which kernels have another name or stand in another file.  Mangled symbols and the function index of block
labels (.LBB<n>_<m>) are normalised; labels, directives and comment lines are not instruction lines."""
import hashlib, os, re, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
from jpeg_amd.build import EXTRA_FLAGS, FLAGS, hipcc   # the flags of the product build
args = sys.argv[1:]
per_kernel = args[:1] == ["--kernels"]
src = args[per_kernel]
cmd = [hipcc(), *FLAGS, *EXTRA_FLAGS.get(os.path.basename(src), []), "-I", os.path.join(root, "include"),
       "--offload-device-only", "-S", src, "-o", "-", *args[per_kernel + 1:]]
proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
if proc.returncode != 0:
    sys.exit(proc.stderr)
lines = [l for l in proc.stdout.splitlines() if "__hip_cuid_" not in l]
if not per_kernel:
    kernels = sum(l.lstrip().startswith(".amdhsa_kernel ") for l in lines)
    print("%-24s %3d kernels %7d lines  sha256 %s" % (os.path.basename(src), kernels, len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()))
    sys.exit(0)
name, body = None, []
for l in lines:
    m = re.match(r"\s*\.type\s+(\S+),@function", l)
    if m:
        name, body = m.group(1), []
    elif name and l.startswith(".Lfunc_end"):
        # (DF16_, _Float16, is newer than many a c++filt: spelled as Dh, which it prints as `half`)
        short = subprocess.run(["c++filt", name.replace("DF16_", "Dh")], capture_output=True, text=True).stdout.strip()
        short = short.replace("jpeg_amd::(anonymous namespace)::", "").replace("jpeg_amd::", "").replace("void ", "", 1)
        short = re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", short)   # the parameter list
        print("%-100s %5d instructions  sha256 %s" % (short, len(body), hashlib.sha256("\n".join(body).encode()).hexdigest()))
        name = None
    elif name and l[:1] in " \t" and l.strip()[:1] not in (".", ";", ""):
        l = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z[\w.$]+", "SYM", l.strip()))
        body.append(re.sub(r"\s+", " ", l))
