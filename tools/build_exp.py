#!/usr/bin/env python3
"""An experimental build of the library beside the product: patched sources and / or extra macros.
    tools/build_exp.py <name> [--patch FILE ...] [-DMACRO ...]   -> tools/exp/libjpeg_amd_<name>.so
    JPEG_AMD_LIBRARY=tools/exp/libjpeg_amd_<name>.so python tools/bench_variants.py ...
The source list and the flags are those of the product build (jpeg_amd.build).  include/ and jpeg_amd/csrc/ are copied to
tools/exp/src_<name>/, the patches are applied to the copy (paths as in the repository: tools/exp_patches/*.diff), every
other argument goes to hipcc.  The instrumentation macros (JA_PHASE_PROFILE, JA_GEN_PHASE, JA_ENC_TIMELINE) need no patch;
the ablation switches need tools/exp_patches/ablation_switches.diff."""
import os, shutil, subprocess, sys
from concurrent.futures import ThreadPoolExecutor
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
from jpeg_amd.build import EXTRA_FLAGS, FLAGS, SOURCES, hipcc   # the product build's sources and flags

args = sys.argv[1:]
if not args or args[0].startswith("-"):
    sys.exit(__doc__)
name, patches, extra = args[0], [], []
rest = iter(args[1:])
for a in rest:
    if a == "--patch":
        patches.append(os.path.abspath(next(rest)))
    else:
        extra.append(a)

top = os.path.join(root, "tools", "exp", "src_" + name)
shutil.rmtree(top, ignore_errors=True)
for d in ("include", os.path.join("jpeg_amd", "csrc")):   # csrc/ reaches the header as ../../include
    shutil.copytree(os.path.join(root, d), os.path.join(top, d), ignore=shutil.ignore_patterns("*.o"))
for p in patches:   # (from the root with --directory: inside a work tree, git apply skips what lies outside its own directory)
    subprocess.check_call(["git", "apply", "--directory=" + os.path.relpath(top, root), "--include=*/include/*", "--include=*/jpeg_amd/csrc/*", p], cwd=root)

cc, csrc = hipcc(), os.path.join(top, "jpeg_amd", "csrc")
def compile_one(src):
    obj = os.path.join(csrc, os.path.splitext(src)[0] + ".o")
    cmd = [cc, *FLAGS, *EXTRA_FLAGS.get(src, []), "-I", os.path.join(top, "include"), *extra, "-c", os.path.join(csrc, src), "-o", obj]
    proc = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if proc.returncode != 0:
        sys.exit("%s:\n%s" % (src, proc.stderr))
    return obj
with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
    objs = list(pool.map(compile_one, SOURCES))
lib = os.path.join(root, "tools", "exp", "libjpeg_amd_%s.so" % name)
subprocess.check_call([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs])
print(lib)
