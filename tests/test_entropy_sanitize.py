"""The host entropy coder under AddressSanitizer + UndefinedBehaviorSanitizer (CPU build only --
GPU sanitizers are not available on the pool): every fixture decoded (1 and 4 threads), written
again as sequential and as progressive scans, decoded again; then 200 corrupted variants each."""
import glob
import os
import platform
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entropy_coder_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "entropy_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "entropy_sanitize.cpp"),
           os.path.join(ROOT, "jpeg_amd", "csrc", "entropy.cpp"), os.path.join(ROOT, "jpeg_amd", "csrc", "entropy_encode.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), *src, "-o", exe, "-lpthread"])
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "decode", "*.jpg")) +
                   glob.glob(os.path.join(ROOT, "tests", "golden", "encode", "*.jpg")))
    assert len(files) >= 25
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *files], capture_output=True, text=True, timeout=1200, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-800:], r.stderr[-2000:])


def test_entropy_decoder_threads_are_clean_under_tsan(tmp_path):
    """The same program under ThreadSanitizer on the fixtures with restart markers, the files whose intervals the decoder
    shares among threads (csrc/entropy.cpp, run_on_threads: the 4-thread decode of the intact file, the 3-thread decode of
    every other damaged copy, the shared clearing of a plane); built and run as the two tests below."""
    exe = str(tmp_path / "entropy_tsan")
    src = [os.path.join(ROOT, "tests", "cpp", "entropy_sanitize.cpp"),
           os.path.join(ROOT, "jpeg_amd", "csrc", "entropy.cpp"), os.path.join(ROOT, "jpeg_amd", "csrc", "entropy_encode.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-I", os.path.join(ROOT, "include"), *src,
                           "-o", exe, "-lpthread"])
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "decode", "*-restart.jpg")))
    assert len(files) >= 3
    r = subprocess.run(["setarch", platform.machine(), "-R", exe, *files], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-800:], r.stderr[-2000:])


def test_worker_pool_is_clean_under_tsan(tmp_path):
    """The host thread pool of the batch file paths (csrc/worker_pool.hpp) under ThreadSanitizer: regions of every size and
    thread limit on pools of 1, 2, 5 and 16 threads -- every item exactly once, never more threads than the region was given,
    begin() / finish() apart -- the directing-thread queue pattern of jpeg_amd_decompress_batch to its end, and the drain of
    its pixels (every byte once, the wait for the download exactly once and before any copy, failure, abandonment)."""
    exe = str(tmp_path / "worker_pool_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-I", os.path.join(ROOT, "jpeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "worker_pool_test.cpp"), "-o", exe, "-lpthread"])
    # GCC's ThreadSanitizer expects the executable and its libraries in fixed address windows; a kernel that randomises
    # mmap with 32 bits (vm.mmap_rnd_bits = 32) can place them outside, and TSan stops before main with "unexpected memory
    # mapping".  The child runs without address-space randomisation (setarch -R: a personality flag of that process only).
    r = subprocess.run(["setarch", platform.machine(), "-R", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-800:], r.stderr[-2000:])


def test_chunk_loop_is_clean_under_tsan(tmp_path):
    """The chunk loop of the batch decodes (csrc/worker_pool.hpp, ChunkLoop) under ThreadSanitizer with a fake device: which
    slot is opened when, the record cursor of a slot, the order of submissions and drains, the three ways a call fails
    (tests/cpp/chunk_loop_test.cpp lists the assertions); built and run as its neighbour above."""
    exe = str(tmp_path / "chunk_loop_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-I", os.path.join(ROOT, "jpeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "chunk_loop_test.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run(["setarch", platform.machine(), "-R", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-800:], r.stderr[-2000:])


def test_tile_staging_is_clean_under_asan_and_ubsan(tmp_path):
    """What the host stages for the tile decode kernels (csrc/tile_staging.hpp) under AddressSanitizer and
    UndefinedBehaviorSanitizer: the region, view and mixed calls' groups against a restatement, and the limit of a grid
    (tests/cpp/tile_staging_test.cpp lists the assertions)."""
    exe = str(tmp_path / "tile_staging_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "jpeg_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "tile_staging_test.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-800:], r.stderr[-2000:])
