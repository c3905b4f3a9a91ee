"""The chunk rule of the resized and tensor decodes (csrc/resample_chunks.hpp) on the host: the stand-alone program
tests/cpp/resample_chunks_test.cpp under AddressSanitizer and UndefinedBehaviorSanitizer (it lists its assertions), and the
splits it prints for the scenarios of test_gpu_resample_chunks against _chunk_seam.expected_chunks -- so that the GPU tests cannot
stop crossing a seam unnoticed when the rule or the constant changes."""
import os
import subprocess

import numpy as np
import pytest

import _chunk_seam as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resample_chunks") / "resample_chunks_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "jpeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "resample_chunks_test.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0 and not r.stderr, (r.stdout[-800:], r.stderr[-2000:])
        return r.stdout
    return run


def printed(program, views, limit=None):
    out = program(*(["--limit", str(limit)] if limit is not None else []), *["%dx%d" % (v[3], v[4]) for v in views])
    return [tuple(int(t) for t in line.split()) for line in out.splitlines()]


def test_chunk_rule_is_clean_under_asan_and_ubsan(program):
    assert program().strip().endswith("ok")


def test_the_python_restatement_is_the_header_on_random_views(program):
    rng = np.random.default_rng(5)
    for _ in range(20):
        views = [(1, 0, 0, int(w), int(h)) for w, h in rng.integers(1, 40, (int(rng.integers(1, 60)), 2))]
        limit = int(rng.integers(1, 9000))
        assert printed(program, views, limit) == S.expected_chunks(views, limit), (views, limit)
    assert printed(program, [(1, 0, 0, 65535, 65535), (1, 0, 0, 1, 1)]) == [(0, 1, 3 * 65535 * 65535), (1, 1, 3)]


def test_the_scenarios_of_the_gpu_tests_cross_their_seams(program):
    """What test_gpu_resample_chunks assumes of each of its calls, by the library's own header."""
    # the mixed calls with views, and the two mapped ones: three chunks, three strides, the places kept in step
    scenarios = [(S.MIXED, S.mixed_views())] + [(S.mapped(p).places, S.mapped(p).views) for p in (False, True)]
    for pl, views in scenarios:
        assert printed(program, views) == S.check_places(pl, views)
        assert len(pl.subset()) >= 10
    assert (S.MIXED.starts, S.MIXED.n, S.MIXED.large) == ((0, 114, 227), 231, (60, 118))
    # views of the small kind cross the seams of the tile grid (128 x 32)
    assert sum(1 for v in S.mixed_views() if v[3] > 128 or v[4] > 32) >= 50
    # the uniform calls: two chunks
    whole, half = 3 * 2048 * 1536, 3 * 1024 * 768
    assert printed(program, S.uniform_views()) == S.expected_chunks(S.uniform_views()) == [(0, 113, whole), (113, 7, half)]
    assert len(S.uniform_subset()) >= 10
    # the refused call: the view past the limit is in the second chunk, and alone in being past it
    views = S.refused_views()
    chunks = printed(program, views)
    assert chunks == S.expected_chunks(views) == [(0, 121, 3 * 1920 * 1536), (121, 19, whole)]
    assert chunks[1][0] <= S.REFUSED_AT < chunks[1][0] + chunks[1][1]
    over = [i for i, v in enumerate(views) if v[3] > 16 * S.REFUSED_CANVAS[0] or v[4] > 16 * S.REFUSED_CANVAS[1]]
    assert over == [S.REFUSED_AT]
