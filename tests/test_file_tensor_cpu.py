"""The file-to-tensor calls without a device: jpeg_amd_spectral_expand_mixed, jpeg_amd_decompress_tensor_mixed and
jpeg_amd_decompress_resized_mixed judge every argument before they look at the context, so a NULL context shows the order of
their checks (in the manner of test_status_order_cpu.py: a call that is right answers the context's EINVAL, one that is
refused for its files or its target answers that verdict); the views and frame infos they return are written in that pass and
are compared with view_denom / view_of_source; and the numpy mirror of the windowed expand's contract (_files.expand_mirror),
which the GPU test compares the kernel with, is checked against the planes jpeg_amd_jpeg_decode_spectral gives.  The file
queue's chunks of different sizes, which the file calls cut, run under ThreadSanitizer in a stand-alone program."""
import ctypes as C
import os
import platform
import subprocess

import numpy as np
import pytest

import _files as F
import jpeg_amd as J
from _calls import FUSED, c_layout, plane_units
from jpeg_amd import _lib

OK, EINVAL, ENOSUP = 0, -1, -5
RGB, BILINEAR, ANTIALIAS = _lib.COLOR_RGB8, _lib.FILTER_BILINEAR, _lib.FILTER_ANTIALIAS


@pytest.fixture(scope="module")
def files():
    return {"420": F.synthetic_file("420", (300, 140), 1)[0], "y8": F.synthetic_file("y8", (131, 257), 2, restart=3)[0],
            "444p": F.synthetic_file("444", (17, 33), 3, kind="progressive")[0],
            "12-bit": F.synthetic_file("y8", (16, 16), 4, precision=12)[0],
            "two": F.synthetic_file(None, (16, 16), 5, factors=[(1, 1), (1, 1)])[0],
            "golden": F.golden_file("color-sequential-restart.jpg")}


def _spec():
    return _lib.TensorSpec(_lib.F16, _lib.TENSOR_CHW, (C.c_float * 3)(1, 2, 3), (C.c_float * 3)(1, 1, 1))


def file_call(datas, regions=None, out=(8, 8), filter=BILINEAR, tensor=True, dst=True, stride=192, spec=True, n=None, color=RGB,
              null_file=None):
    """One of the two file calls with a NULL context -> (status, views [n, 5], infos)."""
    n_files = len(datas)
    ptrs = (C.c_void_p * max(n_files, 1))(*[d.ctypes.data for d in datas])
    if null_file is not None:
        ptrs[null_file] = None
    sizes = (C.c_size_t * max(n_files, 1))(*[d.size for d in datas])
    regs = None
    if regions is not None:
        regs = (_lib.Region * max(n_files, 1))(*[_lib.Region(*r) for r in regions])
    buf = np.zeros(4096, np.uint8)
    infos, views = (_lib.FrameInfo * max(n_files, 1))(), (_lib.View * max(n_files, 1))()
    head = (None, ptrs, sizes, n_files if n is None else n, 1, 0, color, regs, out[0], out[1], filter)
    s = _spec()
    if tensor:
        st = _lib.lib().jpeg_amd_decompress_tensor_mixed(*head, C.byref(s) if spec else None, None, buf.ctypes.data if dst else None,
                                                         stride, infos, views)
    else:
        st = _lib.lib().jpeg_amd_decompress_resized_mixed(*head, buf.ctypes.data if dst else None, stride, infos, views)
    return st, [(v.denom, v.region.x, v.region.y, v.region.width, v.region.height) for v in views], infos


# ---- 1. the order of the checks -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tensor", [True, False], ids=["tensor", "resized"])
def test_status_order_of_the_file_calls(files, tensor):
    good = [files["420"], files["y8"], files["444p"]]
    call = lambda datas, **kw: file_call(datas, tensor=tensor, **kw)[0]   # noqa: E731
    assert call(good) == EINVAL                                        # nothing to refuse: the NULL context, last
    assert call([]) == OK                                              # an empty call needs no context
    assert call([], filter=7) == EINVAL                                # ... but its target is judged
    assert call(good, n=-1) == EINVAL
    assert call(good, n=65536) == EINVAL
    # a file that is not 8-bit with one or three components refuses the whole call, wherever it is
    assert call([files["420"], files["12-bit"], files["y8"]]) == ENOSUP
    assert call([files["420"], files["y8"], files["two"]]) == ENOSUP
    # what is not a JPEG file is what jpeg_amd_jpeg_inspect says of it
    junk = np.zeros(64, np.uint8)
    want = _lib.lib().jpeg_amd_jpeg_inspect(junk.ctypes.data, junk.size, C.byref(_lib.FrameInfo()))
    assert want != OK and call([files["420"], junk]) == want
    assert call(good, null_file=1) == EINVAL
    # a source rectangle outside its image; in index order against a 12-bit file
    whole = [(0, 0, 300, 140), (0, 0, 131, 257), (0, 0, 17, 33)]
    assert call(good, regions=whole) == EINVAL                         # (the context)
    outside = [whole[0], (100, 0, 32, 257), whole[2]]
    assert call([files["420"], files["y8"], files["12-bit"]], regions=outside[:2] + [(0, 0, 16, 16)]) == EINVAL
    assert call([files["12-bit"], files["y8"], files["420"]], regions=[(0, 0, 16, 16), outside[1], whole[0]]) == ENOSUP
    assert call(good, regions=[whole[0], (0, 0, 0, 5), whole[2]]) == EINVAL
    # the target is judged behind the first file, as the mixed calls judge it behind the first image
    assert call([files["12-bit"], files["y8"]], out=(0, 8)) == ENOSUP
    assert call([files["y8"], files["12-bit"]], out=(0, 8)) == EINVAL
    assert call(good, dst=False) == EINVAL
    assert call(good, stride=191) == EINVAL
    assert call(good, filter=7) == EINVAL
    assert call(good, color=9) == EINVAL
    if tensor:
        assert call(good, spec=False) == EINVAL
        assert call([files["12-bit"]], spec=False) == ENOSUP
    # the antialiasing filter's limit is the last verdict: 131 x 257 at denominator 8 is 17 x 33, more than 16 times 1 x 1
    assert call([files["y8"]], out=(1, 1), filter=ANTIALIAS) == ENOSUP
    assert call([files["y8"]], out=(1, 1), filter=BILINEAR) == EINVAL   # (the context)
    assert call([files["y8"], files["12-bit"]], out=(1, 1), filter=ANTIALIAS) == ENOSUP
    assert call([files["y8"], files["y8"]], regions=[(0, 0, 131, 257), (200, 0, 1, 1)], out=(1, 1), filter=ANTIALIAS) == EINVAL


def _item(L, head=8, windows=None, ptr=256):
    it = _lib.ExpandItem()
    it.layout, it.head = L, head
    for p, w in enumerate(windows or F.whole_windows(L)):
        it.d_coef[p] = ptr
        it.window[p] = _lib.Region(*w)
    return it


def test_status_order_of_the_expand():
    L = c_layout(300, 140, FUSED["420"])
    records = np.zeros(16, np.uint32).ctypes.data
    call = lambda it, n=1, rec=records: _lib.lib().jpeg_amd_spectral_expand_mixed(None, n, C.byref(it) if it else None, rec)   # noqa: E731
    assert call(_item(L)) == EINVAL                                    # the NULL context, last
    assert call(_item(L), n=0) == OK and call(None, n=0) == OK         # an empty call needs no context
    # (every refusal below is EINVAL too: what tells it from the context's is test_gpu_expand_mixed.py, with a context)
    assert call(_item(L), n=-1) == EINVAL and call(_item(L), n=65536) == EINVAL
    assert call(None) == EINVAL and call(_item(L), rec=None) == EINVAL
    for head in (0, 2, 3, 16):
        assert call(_item(L, head=head)) == EINVAL


# ---- 2. the views and the frame infos ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out", [(16, 16), (24, 16), (224, 224)])
def test_returned_views_are_the_data_loader_calls(files, out):
    datas = [files["420"], files["y8"], files["444p"], files["golden"]]
    rng = np.random.default_rng(out[0])
    sizes = [(F.inspect(d).width, F.inspect(d).height) for d in datas]
    for regions in (None, [(int(x := rng.integers(0, w)), int(y := rng.integers(0, h)), int(rng.integers(1, w - x + 1)),
                            int(rng.integers(1, h - y + 1))) for w, h in sizes]):
        st, views, infos = file_call(datas, regions=regions, out=out, stride=3 * out[0] * out[1])
        assert st == EINVAL                                            # (the context: everything else was judged, and written)
        for i, (w, h) in enumerate(sizes):
            src = regions[i] if regions else (0, 0, w, h)
            denom = J.view_denom(src[2:], out)
            assert views[i] == (denom,) + J.view_of_source((w, h), denom, src), (i, src)
            assert (infos[i].width, infos[i].height, infos[i].ncomponents) == (w, h, F.inspect(datas[i]).ncomponents)
    assert [F.inspect(d).process for d in datas] == [0, 0, 2, 0]


# ---- 3. the mirror of the expand's contract ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, size, kind, restart", [("420", (300, 140), "sequential", 0), ("y8", (131, 257), "sequential", 3),
                                                       ("422", (17, 33), "scans", 0), ("440", (7, 9), "sequential", 1),
                                                       ("444", (1, 1), "sequential", 0)])
def test_mirror_of_whole_planes_is_the_dense_decode(name, size, kind, restart):
    data, L = F.synthetic_file(name, size, 11, kind, restart)
    st, info, record = F.decode_sparse(data)
    assert st == OK
    _, planes, _ = F.decode_planes(data)
    for got, want in zip(F.expand_mirror(L, record, F.whole_windows(L), 8), planes):
        assert (got == want).all()
    # heads and windows: the head of the window's blocks, the sentinel everywhere else
    windows = [(ux // 2, uy // 3, ux - ux // 2, max(1, uy // 2)) for ux, uy in plane_units(L)]
    for head in (1, 4):
        for got, want, (x, y, w, h) in zip(F.expand_mirror(L, record, windows, head), planes, windows):
            inside = np.zeros(got.shape, bool)
            inside[y:y + h, x:x + w, :8 * head] = True
            assert (got[inside] == want[inside]).all() and (got[~inside] == F.SENTINEL16).all()


def test_mirror_of_the_references_file_is_the_dense_decode():
    data = F.golden_file("color-sequential-restart.jpg")
    st, info, record = F.decode_sparse(data)
    assert st == OK and info.restart_interval > 0
    L = F.layout_of(info)
    _, planes, _ = F.decode_planes(data)
    for got, want in zip(F.expand_mirror(L, record, F.whole_windows(L), 8), planes):
        assert (got == want).all()


def test_the_entries_of_a_block_ascend():
    """What k_expand_mixed's early stop relies on, of the host decoder's records."""
    for data in (F.synthetic_file("420", (300, 140), 1)[0], F.golden_file("color-sequential-restart.jpg")):
        st, info, record = F.decode_sparse(data)
        blocks = sum(info.units_x[c] * info.units_y[c] for c in range(info.ncomponents))
        entries = record[blocks:]
        pos, last = (entries >> 16) & 63, (entries >> 31).astype(bool)
        follows = ~last[:-1]                                           # entry i + 1 belongs to the block of entry i
        assert (pos[1:][follows] > pos[:-1][follows]).all()
        assert (pos[1:][~follows] == 0).all() and pos[0] == 0          # every block begins with its DC


# ---- 4. the file queue with chunks of different sizes ----------------------------------------------------------------------------

def test_file_queue_with_uneven_chunks_is_clean_under_tsan(tmp_path):
    """tests/cpp/file_queue_chunks_test.cpp: every file once, none before its chunk is opened, and a failed call whose
    per-file state outlives the queue that joins the threads (built and run as test_entropy_sanitize.py runs its neighbour)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "file_queue_chunks_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-I", os.path.join(root, "jpeg_amd", "csrc"),
                           os.path.join(root, "tests", "cpp", "file_queue_chunks_test.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run(["setarch", platform.machine(), "-R", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-800:], r.stderr[-2000:])
