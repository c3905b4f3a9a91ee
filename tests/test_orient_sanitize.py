"""csrc/orient.hpp and the EXIF orientation parser (jpeg_amd_jpeg_orientation, csrc/entropy.cpp) under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone CPU program (tests/cpp/orient_sanitize.cpp, built and run as
test_entropy_sanitize.py builds its neighbour): the base and steps of all 8 orientations address every pixel of every small
extent inside the stored image, and the parser answers OK with a value in 1 .. 8 on thousands of truncated and mutated
segments and on every golden file cut at every length below 4 KiB, each in a heap buffer of exactly its size."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_orientation_header_and_parser_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "orient_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "orient_sanitize.cpp"),
           os.path.join(ROOT, "jpeg_amd", "csrc", "entropy.cpp"), os.path.join(ROOT, "jpeg_amd", "csrc", "entropy_encode.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "jpeg_amd", "csrc"), *src, "-o", exe,
                           "-lpthread"])
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "decode", "*.jpg")) +
                   glob.glob(os.path.join(ROOT, "tests", "golden", "encode", "*.jpg")))
    assert len(files) >= 25
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *files], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-800:], r.stderr[-2000:])
