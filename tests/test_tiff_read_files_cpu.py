"""The ``"tiff"`` page kind of ``extractor_batch.read_files`` without a card: the calls it makes on its Reader -- one decode call per shape
group, one for all TIFF pages of a mixed batch, the per-file status, the page-by-page retry, nothing routed differently with the option
off -- pinned with the recording double of test_read_files_cpu.py (CPU tensors stand for device memory; ``tiff_plan`` needs the built
library)."""
import numpy as np
import pytest
import torch

import tiff_decode_ref as R
from test_read_files_cpu import KW, FakeDeviceReader, FakeReader

A, B = (48, 64), (30, 40)
# 10 device-decodable TIFF files (A: 7, B: 3) of all four codecs, a TIFF the plan refuses (16 bit), and a JPEG
SPEC = [("tiff_lzw", A)] * 3 + [("packbits", A)] * 2 + [("tiff_adobe_deflate", B)] * 3 + [("raw", A)] * 2 + [("16bit", A), ("jpg", A)]
MAX_BATCH = 4


class TiffDouble(FakeDeviceReader):
    """... with ``decode_tiff_batch`` / ``decode_tiff_pages``: Pillow stands for the card; ``bad_files``: bytes whose status is non-zero
    (their page is zeroed)"""
    tiff_decode = True

    def __init__(self, fail_tiff=False, **kw):
        super().__init__(**kw)
        self.fail_tiff = fail_tiff

    def _planes(self, pages):
        from bb_ocr_amd.reader import TiffPage, decode_file

        assert all(isinstance(p, TiffPage) for p in pages)
        if self.fail_tiff:
            raise RuntimeError("decode failed")
        bad = [p.data in self.bad_files for p in pages]
        planes = [tuple(np.zeros_like(x) if z else x for x in decode_file(p.data)) for p, z in zip(pages, bad)]
        return planes, [-7 if z else 0 for z in bad]

    def decode_tiff_batch(self, pages):
        pages = list(pages)
        assert all(p.shape == pages[0].shape for p in pages)
        self._note("decode_tiff_batch", (len(pages),) + pages[0].shape)
        planes, status = self._planes(pages)
        return (torch.from_numpy(np.stack([a for a, _ in planes])), torch.from_numpy(np.stack([g for _, g in planes]))), status

    def decode_tiff_pages(self, pages):
        pages = list(pages)
        self._note("decode_tiff_pages", (len(pages),))
        planes, status = self._planes(pages)
        return [(torch.from_numpy(np.array(a)), torch.from_numpy(np.array(g))) for a, g in planes], status


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from PIL import Image

    from bb_ocr_amd.reader import decode_file

    d = tmp_path_factory.mktemp("tiff_read_files")
    rng = np.random.default_rng(8)
    paths = []
    for i, (kind, (h, w)) in enumerate(SPEC):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = d / ("p%02d.%s" % (i, "jpg" if kind == "jpg" else "tiff"))
        if kind == "16bit":
            Image.fromarray(a[..., 0].astype(np.uint16) * 257).save(p)
        elif kind == "jpg":
            Image.fromarray(a).save(p)
        else:
            Image.fromarray(a if i % 2 else a[..., 0]).save(p, compression=kind)
        paths.append(p)
    assert [R.plan(open(p, "rb").read())["supported"] for p in paths] == [1] * 10 + [0, 0]
    ref = FakeReader()
    return paths, {i: ref.texts(*[x[None] for x in decode_file(p)])[0] for i, p in enumerate(paths)}


def run(reader, paths, **kw):
    from bb_ocr_amd import extractor_batch

    return extractor_batch.read_files(reader, paths, None, MAX_BATCH, 4, **kw, **KW)


def calls_of(reader, name):
    return sorted(c[1] for c in reader.calls if c[0] == name)


def test_one_decode_call_per_shape_group(files):
    paths, want = files
    r = TiffDouble()
    assert run(r, paths) == want                                          # tiff_decode: the Reader's
    # groups of one shape, closed at MAX_BATCH pages: A 4 + 3, B 3 -- whatever the codec; every page read from the decoded batch
    assert calls_of(r, "decode_tiff_batch") == [(3, 30, 40, 3), (3, 48, 64, 3), (4, 48, 64, 3)]
    # (the two single pages: the 16-bit file the plan refuses, uploaded as host pixels, and the JPEG file, as its YCbCr triples)
    assert calls_of(r, "readtext_device") == [(1, 48, 64, 3), (1, 48, 64, 3), (3, 30, 40, 3), (3, 48, 64, 3), (4, 48, 64, 3)]
    assert calls_of(r, "_to_dev") and not calls_of(r, "readtext_arrays")


def test_option_off_routes_nothing_differently(files):
    paths, want = files
    off = TiffDouble()
    assert run(off, paths, tiff_decode=False) == want and not calls_of(off, "decode_tiff_batch")
    plain = FakeDeviceReader()                                             # a Reader without the attribute: today's path
    assert run(plain, paths) == want
    assert plain.calls == off.calls or sorted(map(repr, plain.calls)) == sorted(map(repr, off.calls))
    on = FakeDeviceReader()                                                # the keyword alone turns it on: this double cannot decode, so every
    assert run(on, paths, tiff_decode=True) == want                       # TIFF page takes the host decode of its bytes, page by page
    assert len(calls_of(on, "readtext_arrays")) == 10


def test_status_and_page_by_page_retry(files):
    paths, want = files
    bad = {open(paths[1], "rb").read(), open(paths[6], "rb").read()}
    r = TiffDouble(bad_files=bad)
    assert run(r, paths) == want
    assert calls_of(r, "decode_tiff_batch") == [(3, 30, 40, 3), (3, 48, 64, 3), (4, 48, 64, 3)]
    # the two pages of non-zero status are not read from the batch: each takes the host decode of its bytes, alone
    assert calls_of(r, "readtext_device") == [(1, 48, 64, 3), (1, 48, 64, 3), (2, 30, 40, 3), (3, 48, 64, 3), (3, 48, 64, 3)]
    assert calls_of(r, "readtext_arrays") == [(1, 30, 40, 3), (1, 48, 64, 3)]
    f = TiffDouble(fail_tiff=True)                                        # the decode call itself fails: every page of the group, page by page
    assert run(f, paths) == want
    assert len(calls_of(f, "readtext_arrays")) == 10


def test_mixed_batches_decode_every_tiff_page_in_one_call(files, monkeypatch):
    paths, want = files
    monkeypatch.setattr(TiffDouble, "readtext_pages", lambda self, pages, **kw: (self._note("readtext_pages", (len(pages),), kw), self.texts_of(pages))[1],
                        raising=False)
    monkeypatch.setattr(TiffDouble, "texts_of", lambda self, pages: [self.texts(p[0][None].numpy(), p[1][None].numpy())[0] for p in pages], raising=False)
    r = TiffDouble(bad_files={open(paths[0], "rb").read()})
    from bb_ocr_amd import extractor_batch

    assert extractor_batch.read_files(r, paths, None, 64, 4, mixed=True, **KW) == want
    assert calls_of(r, "decode_tiff_pages") == [(10,)] and not calls_of(r, "decode_tiff_batch")       # both shapes, all codecs: one call
    assert calls_of(r, "readtext_pages") == [(11,)] and calls_of(r, "readtext_arrays") == [(1, 48, 64, 3)]
