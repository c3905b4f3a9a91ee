"""The device entropy decoder without a device: the planner's verdicts (jpeg_amd_jpeg_plan_intervals) and the host instantiation
of the kernel's decoder (jpeg_amd_jpeg_decode_intervals_host: csrc/huffman_interval.hpp over the planner's work list) against
jpeg_amd_jpeg_decode_spectral -- exact equality of planes, tables and statuses -- on every fixture, on files written here from
constructed planes and on seeded damage; and the same decoder under AddressSanitizer + UBSan in a program of its own."""
import os
import subprocess

import numpy as np
import pytest

import _entropy_device as E
import _golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_as_host(data):
    """The host form of the kernel's decoder against the host decoder, for a file the planner takes."""
    hs, hinfo, hplanes, hquanta = E.host_decode(data)
    ds, dinfo, dplanes, dquanta = E.intervals_host(data)
    assert ds == hs
    if hs == E.OK:
        assert bytes(dinfo) == bytes(hinfo)
        assert (dquanta == hquanta).all()
        for a, b in zip(dplanes, hplanes):
            assert (a == b).all()
    return hs, dplanes


def test_planner_verdicts_over_all_fixtures():
    verdicts = {n: E.plan(d)[0] for n, d, _ in E.fixture_files()}
    assert len(verdicts) >= 18
    sequential = [n for n in verdicts if "progressive" not in n]
    assert len(sequential) >= 8 and len(verdicts) - len(sequential) >= 8
    assert all(verdicts[n] == (E.OK if n in sequential else E.ENOSUP) for n in verdicts), verdicts


@pytest.mark.parametrize("name,data,entry", E.fixture_files(), ids=[n for n, _, _ in E.fixture_files()])
def test_fixtures(name, data, entry):
    st, nscans, nintervals = E.plan(data)
    hs, info, _, _ = E.host_decode(data)
    assert hs == E.OK
    if info.process == 2:
        assert st == E.ENOSUP
        assert E.intervals_host(data)[0] == E.ENOSUP
        return
    assert st == E.OK and nscans == info.nscans
    mcus = lambda c: info.units_x[c] * info.units_y[c]
    if name == "color-sequential-restart.jpg":
        assert info.restart_interval == 384
    if name == "grayscale-sequential-restart.jpg":
        assert info.restart_interval == 512 and nintervals == -(-mcus(0) // 512)
    if info.restart_interval == 0:
        assert nintervals == nscans
    else:
        assert nintervals > nscans
    status, planes = _same_as_host(data)
    assert status == E.OK
    assert [G.sha(p) for p in planes] == entry["coef_sha256"]


@pytest.mark.parametrize("name", sorted(E.CONSTRUCTED))
def test_constructed_files(name):
    data, planes = E.constructed_file(name)
    layout, size, restart, kind, precision = E.CONSTRUCTED[name]
    st, nscans, nintervals = E.plan(data)
    assert st == E.OK
    assert nscans == (len(planes) if kind == "scans" else 1)
    status, got = _same_as_host(data)
    assert status == E.OK
    for a, b in zip(got, planes):                     # the file holds the planes it was written from
        assert (a == b).all()
    if "65-intervals" in name:
        assert nintervals == 65
    if "257-intervals" in name:
        assert nintervals == 257
    if name == "420-64x48-ri1":
        assert nintervals == 12                       # RST0 .. RST7 and round again


def test_constructed_files_take_every_path():
    """What the constructed planes are for is in the STREAMS, counted symbol by symbol by a plain reader of the test's own
    (E.stream_stats), in files that the planner takes and the kernel's decoder decodes to the planes they were written from."""
    total = {}
    for name in sorted(E.CONSTRUCTED):
        data, planes = E.constructed_file(name)
        assert E.plan(data)[0] == E.OK
        st, _, got, _ = E.intervals_host(data)
        assert st == E.OK and all((a == b).all() for a, b in zip(got, planes))
        stats = E.stream_stats(data)
        assert stats["blocks"] >= sum(p.shape[0] * p.shape[1] for p in planes)          # (an interleaved scan pads its MCUs)
        for key, v in stats.items():
            total[key] = max(total.get(key, 0), v) if key.startswith(("longest", "dc_size")) else total.get(key, 0) + v
        if E.CONSTRUCTED[name][4] == 8:
            assert stats["dc_size"] <= 11
            total["dc_size_8bit"] = max(total.get("dc_size_8bit", 0), stats["dc_size"])
        assert stats["zrl_before_eob"] >= 1 and stats["long_runs"] >= 1 and stats["no_eob"] >= 1, (name, stats)
        assert any((p.reshape(-1, 64) == 0).all(1).any() for p in planes), name       # an all-zero block
    assert total["longest_code"] >= 10                  # codes beyond the 9-bit first level are read ...
    assert total["longest_code_and_magnitude"] >= 17    # ... and symbols that no 10-bit window holds
    assert total["dc_size_8bit"] == 11                  # a DC difference of size 11 is read (where an interval holds two blocks)
    assert total["dc_size"] >= 12                       # (the 12-bit files)
    assert total["stuffed"] >= 20                       # FF 00 pairs: a small file may hold none, the set holds many


def test_a_component_that_two_scans_write_is_left_to_the_host():
    """The one refusal beyond jpeg_amd_jpeg_decode_sparse's: the host decodes scans in order and the later one wins."""
    base = E.constructed_file("420-35x19-scans-ri2")[0]
    twice = E.twice_scanned(base)
    assert E.plan(base)[0] == E.OK
    assert E.host_decode(twice)[0] == E.OK
    assert E.plan(twice)[0] == E.ENOSUP and E.intervals_host(twice)[0] == E.ENOSUP


@pytest.mark.parametrize("name", ["420-64x48-row", "grey-35x19-ri2", "420-35x19-scans-ri2", "four-12bit-35x19-ri2"])
def test_a_dc_symbol_above_16_is_the_interval_status(name):
    """The one status an interval can have besides OK, on a file built to have it: the planner takes the file, and the host
    form of the kernel's decoder reduces its intervals to the host decoder's EINVAL."""
    bad = E.dc_symbol_17(E.constructed_file(name)[0])
    assert E.plan(bad)[0] == E.OK
    assert E.host_decode(bad)[0] == E.EINVAL
    assert E.intervals_host(bad)[0] == E.EINVAL


@pytest.mark.parametrize("case", range(len(E.damaged_files())), ids=[n for n, _, _ in E.damaged_files()])
def test_seeded_damage(case):
    name, data, verdict = E.damaged_files()[case]
    st, _, _ = E.plan(data)
    assert st == verdict
    if st == E.OK:
        _same_as_host(data)                           # (a status that is not OK included: then the statuses are compared)
    else:
        ds, _, planes, _ = E.intervals_host(data)
        assert ds == st
        if planes is not None:
            assert all((p == -23131).all() for p in planes)       # refused: nothing written


def test_undefined_tables_and_unbound_quanta_are_malformed():
    import _files as F
    data = E.constructed_file("420-64x48-row")[0]
    assert E.plan(F.undefined_tables(data))[0] == E.EINVAL
    assert E.host_decode(F.undefined_tables(data))[0] == E.EINVAL
    bad = data.copy()
    dqt = bytes(bad).index(b"\xff\xdb")
    bad[dqt + 1] = 0xFE                                # the DQT segment becomes a comment: no table is ever defined
    assert E.plan(bad)[0] == E.EINVAL and E.host_decode(bad)[0] == E.EINVAL
    assert E.plan(F.lossless_marker(data))[0] == E.ENOSUP
    assert E.plan(np.zeros(16, np.uint8))[0] == E.EINVAL


def test_host_instantiation_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/cpp/entropy_device_host.cpp: the planner and the host instantiation of the decoder on the damaged files above
    and the files they were made from, each in a heap allocation of exactly its size, under AddressSanitizer and UBSan."""
    exe = str(tmp_path / "entropy_device_host")
    src = [os.path.join(ROOT, "tests", "cpp", "entropy_device_host.cpp"),
           os.path.join(ROOT, "jpeg_amd", "csrc", "entropy.cpp"), os.path.join(ROOT, "jpeg_amd", "csrc", "entropy_encode.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), *src, "-o", exe, "-lpthread"])
    files = []
    cases = [(n, d) for n, d, _ in E.damaged_files()] + [(n, E.constructed_file(n)[0]) for n in sorted(E.CONSTRUCTED)]
    for k, (name, data) in enumerate(cases):
        path = tmp_path / f"{k:03d}.jpg"
        data.tofile(path)
        files.append(str(path))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *files], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-800:], r.stderr[-2000:])
