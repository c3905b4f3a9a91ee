"""What the host entropy decoder writes for damaged files, progressive ones included, held to a record: status and SHA-256 of
the planes and tables (one thread; the careful reader; on the intact file the previews after 1 and 2 scans) and of the raw
sparse record, for the intact file and 16 damaged copies of every tests/golden/decode/*.jpg.  The copies come from the
generator's own code (tests/golden/make_entropy_damaged.py), the expectations from its output.  CPU only."""
import importlib.util
import json
import os

import pytest

import _golden as G
from jpeg_amd import _lib

_spec = importlib.util.spec_from_file_location("make_entropy_damaged", G.path("make_entropy_damaged.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

with open(M.FIXTURE) as _f:
    FIXTURE = json.load(_f)


def test_the_fixture_covers_every_decode_file():
    assert sorted(FIXTURE["files"]) == [os.path.basename(p) for p in M.files()]
    assert (FIXTURE["seed"], FIXTURE["copies"], FIXTURE["kinds"]) == (M.SEED, M.COPIES, M.KINDS)
    assert os.path.getsize(M.FIXTURE) < 100_000


@pytest.mark.parametrize("name", sorted(FIXTURE["files"]))
def test_damaged_files_decode_to_the_recorded_status_and_bytes(name):
    lib = _lib.lib()
    data = open(G.path(os.path.join("decode", name)), "rb").read()
    info = M.inspect(lib, data)
    want = FIXTURE["files"][name]
    made = list(M.copies(data, name))
    assert len(made) == len(want) == 1 + M.COPIES
    for i, ((kind, d), w) in enumerate(zip(made, want)):
        assert kind == w["kind"]
        got = M.record(lib, d, info, kind == 0)
        for call, (status, sha) in got.items():
            assert [status, sha] == w[call], (name, i, M.KINDS[kind], call)
        assert sorted(got) == sorted(k for k in w if k != "kind")
        if info.restart_interval and kind != M.REMOVED_MARKER:
            one = M.decode_planes(lib, d, info)
            three = M.decode_planes(lib, d, info, threads=3)
            assert three[0] == one[0], (name, i, M.KINDS[kind])
            if one[0] == 0:
                assert all((p == q).all() for p, q in zip(three[1], one[1])), (name, i, M.KINDS[kind])
