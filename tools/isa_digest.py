#!/usr/bin/env python3
"""Kernel count and SHA-256 of the gfx950 device assembly of a .hip file, compiled with the product flags:
    tools/isa_digest.py jpeg_amd/csrc/kernels_quad.hip [-DMACRO ...]
Equal digests before and after a refactor mean the same instructions, registers and LDS: no kernel changed.  The lines that
contain __hip_cuid_ are left out (that symbol hashes the source text); nothing else of the assembly is looked at."""
import hashlib, os, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
from jpeg_amd.build import EXTRA_FLAGS, FLAGS, hipcc   # the flags of the product build
src = sys.argv[1]
cmd = [hipcc(), *FLAGS, *EXTRA_FLAGS.get(os.path.basename(src), []), "-I", os.path.join(root, "include"),
       "--offload-device-only", "-S", src, "-o", "-", *sys.argv[2:]]
proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
if proc.returncode != 0:
    sys.exit(proc.stderr)
lines = [l for l in proc.stdout.splitlines() if "__hip_cuid_" not in l]
kernels = sum(l.lstrip().startswith(".amdhsa_kernel ") for l in lines)
print("%-24s %3d kernels %7d lines  sha256 %s" % (os.path.basename(src), kernels, len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()))
