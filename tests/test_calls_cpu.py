"""The sentinel check the GPU tests of the batch calls rely on (_calls.assert_only_spans_written), on numpy buffers -- no GPU and
no library: it passes for a clean buffer and fails on one stray byte in each place the calls must leave alone."""
import numpy as np
import pytest

from _calls import SENTINEL, assert_only_spans_written, out_spans

COUNTS = [5, 12, 1, 7]                                      # elements per image: they differ, as in a view or region call
GAP, LEAD, TAIL = 3, 2, 4                                   # in elements


def _buffer(elem):
    """The buffer of _calls.Out on the host: -> (bytes, spans), every image's bytes written (to a value that is not the
    sentinel, and with the sentinel's own value at one place inside an image: that must not matter)."""
    stride, nbytes, spans = out_spans(COUNTS, elem, GAP, LEAD, TAIL)
    assert stride == 15 and nbytes == (LEAD + 4 * 15 + TAIL) * elem and spans[0] == (LEAD * elem, 5 * elem)
    assert all(b[0] - (a[0] + a[1]) >= GAP * elem for a, b in zip(spans, spans[1:]))
    host = np.full(nbytes, SENTINEL, np.uint8)
    for a, m in spans:
        host[a:a + m] = 0x11
    host[spans[1][0] + 1] = SENTINEL
    return host, spans


@pytest.mark.parametrize("elem", [1, 2, 4])
def test_a_clean_buffer_passes(elem):
    host, spans = _buffer(elem)
    assert_only_spans_written(host, spans)
    assert_only_spans_written(np.full(7, SENTINEL, np.uint8), [])          # a refused call: nothing written at all
    assert_only_spans_written(host, spans, sentinel=SENTINEL)


@pytest.mark.parametrize("where", ["gap", "last byte of a gap", "tail", "last byte of the tail", "lead", "first byte"])
@pytest.mark.parametrize("elem", [1, 2, 4])
def test_one_stray_byte_fails(elem, where):
    host, spans = _buffer(elem)
    at = {"gap": spans[0][0] + spans[0][1],                 # the first byte behind image 0, the shortest before a long gap
          "last byte of a gap": spans[2][0] - 1,            # directly in front of image 2
          "tail": spans[-1][0] + spans[-1][1],              # the first byte behind the last image
          "last byte of the tail": host.size - 1,
          "lead": spans[0][0] - 1,                          # directly in front of image 0
          "first byte": 0}[where]
    assert all(not a <= at < a + m for a, m in spans)
    host[at] ^= 0x01
    with pytest.raises(AssertionError):
        assert_only_spans_written(host, spans)
    host[at] ^= 0x01
    assert_only_spans_written(host, spans)


def test_a_write_inside_an_image_is_not_its_business():
    host, spans = _buffer(2)
    for a, m in spans:
        host[a], host[a + m - 1] = 0, 0xFF
    assert_only_spans_written(host, spans)
