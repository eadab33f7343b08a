"""tests/views.py on the CPU: rows survive embed -> extract in every geometry class, and outside_untouched fails on one
flipped byte of every region it guards -- without that, the canary assertions of tests/test_ops_views_gpu.py could pass
vacuously."""
import numpy as np
import pytest

import views
from views import CLASSES, GUARD, HEAD

ROW_BYTES = [272, 512, 34, 4]          # Q8 rows of 256, f16 rows of 256, one Q8 block, one dword


def _rows(seed, n, row_bytes):
    return np.random.default_rng(seed).integers(0, 256, (n, row_bytes), dtype=np.uint8)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_rows_round_trip(cls, row_bytes):
    off, pad = cls
    n, pitch = 5, row_bytes + pad
    rows = _rows(off * 100 + pad + row_bytes, n, row_bytes)
    parent = views.embed(rows, off, pitch, 0xA5)
    assert parent.dtype == np.uint8 and parent.size == HEAD + off + n * pitch + GUARD
    assert np.array_equal(views.extract(parent, off, pitch, n, row_bytes), rows)
    # row r lies at HEAD + offset + r * pitch, and nothing else of the parent holds rows
    for r in range(n):
        assert np.array_equal(parent[HEAD + off + r * pitch:][:row_bytes], rows[r])
    blank = views.embed(np.zeros_like(rows), off, pitch, 0xA5)
    same = parent == blank
    inside = np.zeros(parent.size, bool)
    for r in range(n):
        inside[HEAD + off + r * pitch:][:row_bytes] = True
    assert same[~inside].all(), "canaries depend on the position only"
    assert len(np.unique(blank[:HEAD])) == 256, "a stray store of any constant byte meets a canary that differs from it"


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("start_pos", [0, 2])
def test_outside_untouched_passes_on_written_rows_only(cls, start_pos):
    off, pad = cls
    n, row_bytes = 4, 272
    pitch = row_bytes + pad
    before = views.embed(_rows(1, n, row_bytes), off, pitch, 0x3C)
    views.outside_untouched(before, before.copy(), off, pitch, n, row_bytes, start_pos)
    after = before.copy()
    for r in range(start_pos, n):                                    # every byte of every written row changes
        after[HEAD + off + r * pitch:][:row_bytes] ^= 0xFF
    views.outside_untouched(before, after, off, pitch, n, row_bytes, start_pos)
    assert np.array_equal(views.extract(after, off, pitch, n, row_bytes)[:start_pos], views.extract(before, off, pitch, n, row_bytes)[:start_pos])


def _regions(off, pad, n, row_bytes, start_pos):
    """(name, parent byte) of one byte in every region outside the written rows; the first and the last byte of each"""
    pitch = row_bytes + pad
    b = HEAD + off
    end = b + n * pitch
    out = [("guard before", b - GUARD), ("guard before, last byte", b - 1), ("guard behind", end), ("guard behind, last byte", end + GUARD - 1),
           ("the parent's first byte", 0)]
    if pad:
        out += [("padding of the first written row", b + start_pos * pitch + row_bytes), ("padding of a row, last byte", b + (start_pos + 1) * pitch - 1),
                ("padding of the last row", b + (n - 1) * pitch + row_bytes), ("padding of the last row, last byte", end - 1)]
    if start_pos:
        out += [("row 0, below start_pos", b), ("the last byte below start_pos", b + (start_pos - 1) * pitch + row_bytes - 1)]
        if pad:
            out += [("padding below start_pos", b + (start_pos - 1) * pitch + row_bytes)]
    return out


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("start_pos", [0, 1, 3])
def test_outside_untouched_fails_on_one_flipped_byte_of_every_region(cls, start_pos):
    off, pad = cls
    n, row_bytes = 4, 34
    pitch = row_bytes + pad
    before = views.embed(_rows(2, n, row_bytes), off, pitch, 0x11)
    regions = _regions(off, pad, n, row_bytes, start_pos)
    assert {r[0] for r in regions} >= {"guard before", "guard behind"}
    for name, i in regions:
        for flip in (0x01, 0x80):
            after = before.copy()
            after[i] ^= flip
            with pytest.raises(AssertionError, match="outside the written rows"):
                views.outside_untouched(before, after, off, pitch, n, row_bytes, start_pos, what=name)
    # ... and the neighbours of those bytes INSIDE the written rows are free
    after = before.copy()
    after[HEAD + off + start_pos * pitch] ^= 1
    after[HEAD + off + (n - 1) * pitch + row_bytes - 1] ^= 1
    views.outside_untouched(before, after, off, pitch, n, row_bytes, start_pos)


def test_outside_untouched_wants_the_whole_parent():
    before = views.embed(_rows(3, 2, 34), 2, 36, 0)
    with pytest.raises(AssertionError):
        views.outside_untouched(before, before[:-1], 2, 36, 2, 34)
    with pytest.raises(AssertionError):
        views.extract(before[:-GUARD], 2, 36, 2, 34)
