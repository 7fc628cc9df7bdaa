"""The ``"png"`` page kind of ``extractor_batch.read_files`` without a card: the calls it makes on its Reader -- one decode call per shape
group, the per-file status, the page-by-page retry -- pinned with the recording double of test_read_files_cpu.py (CPU tensors stand for
device memory; ``png_plan`` needs the built library)."""

import numpy as np
import pytest
import torch

import png_decode_ref as R
from test_read_files_cpu import KW, FakeDeviceReader, FakeReader

A, B = (48, 64), (30, 40)
SPEC = [("rgb", A)] * 5 + [("L", B)] * 3 + [("1bit", A)] * 2 + [("adam7", A), ("jpg", A)]      # 10 device-decodable PNG files, A: 7, B: 3
MAX_BATCH = 4


class PngDouble(FakeDeviceReader):
    """... with ``decode_png_batch``: Pillow stands for the card; ``bad_files``: bytes whose status is non-zero (their page is zeroed)"""
    png_decode = True

    def __init__(self, fail_png=False, **kw):
        super().__init__(**kw)
        self.fail_png = fail_png

    def decode_png_batch(self, pages):
        from bb_ocr_amd.reader import PngPage, decode_file

        pages = list(pages)
        assert all(isinstance(p, PngPage) and p.shape == pages[0].shape for p in pages)
        self._note("decode_png_batch", (len(pages),) + pages[0].shape)
        if self.fail_png:
            raise RuntimeError("decode failed")
        planes = [decode_file(p.data) for p in pages]
        bad = [p.data in self.bad_files for p in pages]
        rgb = np.stack([np.zeros_like(a) if z else a for (a, _), z in zip(planes, bad)])
        gray = np.stack([np.zeros_like(g) if z else g for (_, g), z in zip(planes, bad)])
        return (torch.from_numpy(rgb), torch.from_numpy(gray)), [-7 if z else 0 for z in bad]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from PIL import Image

    from bb_ocr_amd.reader import decode_file

    d = tmp_path_factory.mktemp("png_read_files")
    rng = np.random.default_rng(8)
    paths = []
    for i, (kind, (h, w)) in enumerate(SPEC):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = d / ("p%02d.%s" % (i, "jpg" if kind == "jpg" else "png"))
        if kind == "adam7":
            p.write_bytes(R.adam7_file(a))
        else:
            Image.fromarray(a if kind in ("rgb", "jpg") else (a[..., 0] if kind == "L" else a[..., 0] > 127)).save(p)
        paths.append(p)
    ref = FakeReader()
    return paths, {i: ref.texts(*[x[None] for x in decode_file(p)])[0] for i, p in enumerate(paths)}


def run(reader, paths, **kw):
    from bb_ocr_amd import extractor_batch

    return extractor_batch.read_files(reader, paths, None, MAX_BATCH, 4, **kw, **KW)


def calls_of(reader, name):
    return sorted(c[1] for c in reader.calls if c[0] == name)


def test_one_decode_call_per_shape_group(files):
    paths, want = files
    r = PngDouble()
    assert run(r, paths) == want                                          # png_decode: the Reader's
    # groups of one shape, closed at MAX_BATCH pages: A 4 + 3, B 3; every page read from the decoded batch by one device call per group
    assert calls_of(r, "decode_png_batch") == [(3, 30, 40, 3), (3, 48, 64, 3), (4, 48, 64, 3)]
    # (the two single pages: the Adam7 file, uploaded as host pixels, and the JPEG file, uploaded as its YCbCr triples)
    assert calls_of(r, "readtext_device") == [(1, 48, 64, 3), (1, 48, 64, 3), (3, 30, 40, 3), (3, 48, 64, 3), (4, 48, 64, 3)]
    assert calls_of(r, "_to_dev") and not calls_of(r, "readtext_arrays")
    off = PngDouble()
    assert run(off, paths, png_decode=False) == want and not calls_of(off, "decode_png_batch")


def test_status_and_page_by_page_retry(files):
    paths, want = files
    bad = {open(paths[1], "rb").read(), open(paths[6], "rb").read()}
    r = PngDouble(bad_files=bad)
    assert run(r, paths) == want
    assert calls_of(r, "decode_png_batch") == [(3, 30, 40, 3), (3, 48, 64, 3), (4, 48, 64, 3)]
    # the two pages of non-zero status are not read from the batch: each takes the host decode of its bytes, alone
    assert calls_of(r, "readtext_device") == [(1, 48, 64, 3), (1, 48, 64, 3), (2, 30, 40, 3), (3, 48, 64, 3), (3, 48, 64, 3)]
    assert calls_of(r, "readtext_arrays") == [(1, 30, 40, 3), (1, 48, 64, 3)]
    f = PngDouble(fail_png=True)                                          # the decode call itself fails: every page of the group, page by page
    assert run(f, paths) == want
    assert len(calls_of(f, "readtext_arrays")) == 10


def test_mixed_batches_group_png_pages_by_shape(files, monkeypatch):
    paths, want = files
    monkeypatch.setattr(PngDouble, "readtext_pages", lambda self, pages, **kw: (self._note("readtext_pages", (len(pages),), kw), self.texts_of(pages))[1],
                        raising=False)
    monkeypatch.setattr(PngDouble, "texts_of", lambda self, pages: [self.texts(p[0][None].numpy(), p[1][None].numpy())[0] for p in pages], raising=False)
    r = PngDouble(bad_files={open(paths[0], "rb").read()})
    from bb_ocr_amd import extractor_batch

    assert extractor_batch.read_files(r, paths, None, 64, 4, mixed=True, **KW) == want
    assert calls_of(r, "decode_png_batch") == [(3, 30, 40, 3), (7, 48, 64, 3)]          # one call per shape inside the one mixed batch
    assert calls_of(r, "readtext_pages") == [(11,)] and calls_of(r, "readtext_arrays") == [(1, 48, 64, 3)]
