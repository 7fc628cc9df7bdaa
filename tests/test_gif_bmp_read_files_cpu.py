"""The ``"gif"`` page kind of ``extractor_batch.read_files`` without a card: the calls it makes on its Reader -- one decode call per shape
group, one for all GIF pages of a mixed batch, the per-file status, the page-by-page retry, nothing routed differently with the option off
-- pinned with the recording double of test_read_files_cpu.py (CPU tensors stand for device memory; ``gif_plan`` needs the built library)."""
import numpy as np
import pytest
import torch

import gif_decode_ref as R
from test_read_files_cpu import KW, FakeDeviceReader, FakeReader

A, B = (48, 64), (30, 40)
# 8 device-decodable GIF files (A: 5, B: 3), a GIF the plan refuses (no terminator), and a JPEG
SPEC = [("L", A)] * 2 + [("P", A)] * 2 + [("interlaced", B)] * 3 + [("1bit", A), ("refused", A), ("jpg", A)]
MAX_BATCH = 4


class GifDouble(FakeDeviceReader):
    """... with ``decode_gif_pages``: Pillow stands for the card; ``bad_files``: bytes whose status is non-zero (their page is zeroed)"""
    gif_decode = True

    def __init__(self, fail_gif=False, **kw):
        super().__init__(**kw)
        self.fail_gif = fail_gif

    def decode_gif_pages(self, pages):
        from bb_ocr_amd.reader import GifPage, decode_file

        pages = list(pages)
        assert all(isinstance(p, GifPage) for p in pages)
        self._note("decode_gif_pages", (len(pages),) + (pages[0].shape if all(p.shape == pages[0].shape for p in pages) else ()))
        if self.fail_gif:
            raise RuntimeError("decode failed")
        bad = [p.data in self.bad_files for p in pages]
        planes = [tuple(np.zeros_like(x) if z else x for x in decode_file(p.data)) for p, z in zip(pages, bad)]
        return [(torch.from_numpy(np.array(a)), torch.from_numpy(np.array(g))) for a, g in planes], [-7 if z else 0 for z in bad]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from PIL import Image

    from bb_ocr_amd.reader import decode_file

    d = tmp_path_factory.mktemp("gif_read_files")
    rng = np.random.default_rng(8)
    paths = []
    for i, (kind, (h, w)) in enumerate(SPEC):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = d / ("p%02d.%s" % (i, "jpg" if kind == "jpg" else "gif"))
        if kind == "jpg":
            Image.fromarray(a).save(p)
        else:
            pil = Image.fromarray(a if kind == "P" else (a[..., 0] > 127 if kind == "1bit" else a[..., 0]))
            f = R.pillow_file(pil, interlace=int(kind == "interlaced"))
            p.write_bytes(f[:-2] if kind == "refused" else f)
        paths.append(p)
    assert [R.plan(open(p, "rb").read())["supported"] for p in paths] == [1] * 8 + [0, 0]
    ref = FakeReader()
    return paths, {i: ref.texts(*[x[None] for x in decode_file(p)])[0] for i, p in enumerate(paths)}


def run(reader, paths, **kw):
    from bb_ocr_amd import extractor_batch

    return extractor_batch.read_files(reader, paths, None, MAX_BATCH, 4, **kw, **KW)


def calls_of(reader, name):
    return sorted(c[1] for c in reader.calls if c[0] == name)


def test_one_decode_call_per_shape_group(files):
    paths, want = files
    r = GifDouble()
    assert run(r, paths) == want                                          # gif_decode: the Reader's
    # groups of one shape, closed at MAX_BATCH pages: A 4 + 1, B 3 -- gray, palette and 1-bit pages alike; every page read from the planes
    assert calls_of(r, "decode_gif_pages") == [(1, 48, 64, 3), (3, 30, 40, 3), (4, 48, 64, 3)]
    # (the two single pages: the file the plan refuses, uploaded as host pixels, and the JPEG file, as its YCbCr triples)
    assert calls_of(r, "readtext_device") == [(1, 48, 64, 3), (1, 48, 64, 3), (1, 48, 64, 3), (3, 30, 40, 3), (4, 48, 64, 3)]
    assert calls_of(r, "_to_dev") and not calls_of(r, "readtext_arrays")


def test_option_off_routes_nothing_differently(files):
    paths, want = files
    off = GifDouble()
    assert run(off, paths, gif_decode=False) == want and not calls_of(off, "decode_gif_pages")
    plain = FakeDeviceReader()                                             # a Reader without the attribute: today's path
    assert run(plain, paths) == want
    assert plain.calls == off.calls or sorted(map(repr, plain.calls)) == sorted(map(repr, off.calls))
    on = FakeDeviceReader()                                                # the keyword alone turns it on: this double cannot decode, so every
    assert run(on, paths, gif_decode=True) == want                        # GIF page takes the host decode of its bytes, page by page
    assert len(calls_of(on, "readtext_arrays")) == 8


def test_status_and_page_by_page_retry(files):
    paths, want = files
    bad = {open(paths[1], "rb").read(), open(paths[5], "rb").read()}
    r = GifDouble(bad_files=bad)
    assert run(r, paths) == want
    assert calls_of(r, "decode_gif_pages") == [(1, 48, 64, 3), (3, 30, 40, 3), (4, 48, 64, 3)]
    # the two pages of non-zero status are not read from the planes: each takes the host decode of its bytes, alone
    assert calls_of(r, "readtext_device") == [(1, 48, 64, 3), (1, 48, 64, 3), (1, 48, 64, 3), (2, 30, 40, 3), (3, 48, 64, 3)]
    assert calls_of(r, "readtext_arrays") == [(1, 30, 40, 3), (1, 48, 64, 3)]
    f = GifDouble(fail_gif=True)                                          # the decode call itself fails: every page of the group, page by page
    assert run(f, paths) == want
    assert len(calls_of(f, "readtext_arrays")) == 8


def test_mixed_batches_decode_every_gif_page_in_one_call(files, monkeypatch):
    paths, want = files
    monkeypatch.setattr(GifDouble, "readtext_pages", lambda self, pages, **kw: (self._note("readtext_pages", (len(pages),), kw), self.texts_of(pages))[1],
                        raising=False)
    monkeypatch.setattr(GifDouble, "texts_of", lambda self, pages: [self.texts(p[0][None].numpy(), p[1][None].numpy())[0] for p in pages], raising=False)
    r = GifDouble(bad_files={open(paths[0], "rb").read()})
    from bb_ocr_amd import extractor_batch

    assert extractor_batch.read_files(r, paths, None, 64, 4, mixed=True, **KW) == want
    assert calls_of(r, "decode_gif_pages") == [(8,)]                      # both shapes: one call
    assert calls_of(r, "readtext_pages") == [(9,)] and calls_of(r, "readtext_arrays") == [(1, 48, 64, 3)]


# ------------------------------------------------------------------------------------------------ the "bmp" kind
import bmp_decode_ref as RB

# 7 device-decodable BMP files (A: 4, B: 3), a BMP the plan refuses (RLE8), and a JPEG
BMP_SPEC = [("RGB", A)] * 2 + [("L", B)] * 2 + [("P", A), ("1bit", A), ("RGBA", B), ("rle", A), ("jpg", A)]


class BmpDouble(FakeDeviceReader):
    """... with ``decode_bmp_pages``: Pillow stands for the card; ``bad_files``: bytes whose status is non-zero"""
    bmp_decode = True

    def decode_bmp_pages(self, pages):
        from bb_ocr_amd.reader import BmpPage, decode_file

        pages = list(pages)
        assert all(isinstance(p, BmpPage) for p in pages)
        self._note("decode_bmp_pages", (len(pages),) + (pages[0].shape if all(p.shape == pages[0].shape for p in pages) else ()))
        bad = [p.data in self.bad_files for p in pages]
        planes = [tuple(np.zeros_like(x) if z else x for x in decode_file(p.data)) for p, z in zip(pages, bad)]
        return [(torch.from_numpy(np.array(a)), torch.from_numpy(np.array(g))) for a, g in planes], [-1 if z else 0 for z in bad]


@pytest.fixture(scope="module")
def bmp_files(tmp_path_factory):
    from PIL import Image

    from bb_ocr_amd.reader import decode_file

    d = tmp_path_factory.mktemp("bmp_read_files")
    rng = np.random.default_rng(9)
    paths = []
    for i, (kind, (h, w)) in enumerate(BMP_SPEC):
        a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        p = d / ("p%02d.%s" % (i, "jpg" if kind == "jpg" else "bmp"))
        if kind == "jpg":
            Image.fromarray(a[..., :3]).save(p)
        elif kind == "rle":
            p.write_bytes(RB.rle8_file(a[..., 0], RB.colour_table(256, 1)))
        else:
            pil = {"RGB": Image.fromarray(a[..., :3]), "L": Image.fromarray(a[..., 0]), "P": Image.fromarray(a[..., :3]).quantize(64),
                   "1bit": Image.fromarray(a[..., 0] > 127), "RGBA": Image.fromarray(a)}[kind]
            p.write_bytes(RB.pillow_file(pil))
        paths.append(p)
    assert [RB.plan(open(p, "rb").read())["supported"] for p in paths] == [1] * 7 + [0, 0]
    ref = FakeReader()
    return paths, {i: ref.texts(*[x[None] for x in decode_file(p)])[0] for i, p in enumerate(paths)}


def test_bmp_one_decode_call_per_shape_group_and_retry(bmp_files):
    paths, want = bmp_files
    r = BmpDouble()
    assert run(r, paths) == want                                          # bmp_decode: the Reader's
    assert calls_of(r, "decode_bmp_pages") == [(3, 30, 40, 3), (4, 48, 64, 3)]
    # (the two single pages: the RLE file the plan refuses, decoded by Pillow and uploaded as pixels, and the JPEG file)
    assert calls_of(r, "readtext_device") == [(1, 48, 64, 3), (1, 48, 64, 3), (3, 30, 40, 3), (4, 48, 64, 3)]
    assert not calls_of(r, "readtext_arrays")
    b = BmpDouble(bad_files={open(paths[2], "rb").read()})                # a page of non-zero status takes the host decode of its bytes, alone
    assert run(b, paths) == want
    assert calls_of(b, "readtext_device") == [(1, 48, 64, 3), (1, 48, 64, 3), (2, 30, 40, 3), (4, 48, 64, 3)] and calls_of(b, "readtext_arrays") == [(1, 30, 40, 3)]


def test_bmp_option_off_routes_nothing_differently(bmp_files):
    paths, want = bmp_files
    off = BmpDouble()
    assert run(off, paths, bmp_decode=False) == want and not calls_of(off, "decode_bmp_pages")
    plain = FakeDeviceReader()                                             # a Reader without the attribute: today's path
    assert run(plain, paths) == want
    assert plain.calls == off.calls or sorted(map(repr, plain.calls)) == sorted(map(repr, off.calls))
    on = FakeDeviceReader()                                                # the keyword alone turns it on: this double cannot decode
    assert run(on, paths, bmp_decode=True) == want
    assert len(calls_of(on, "readtext_arrays")) == 7


def test_gif_and_bmp_pages_of_a_mixed_batch_take_one_call_each(files, bmp_files, monkeypatch):
    (gif_paths, gif_want), (bmp_paths, bmp_want) = files, bmp_files

    class Both(GifDouble, BmpDouble):
        pass

    monkeypatch.setattr(Both, "readtext_pages", lambda self, pages, **kw: (self._note("readtext_pages", (len(pages),), kw), self.texts_of(pages))[1],
                        raising=False)
    monkeypatch.setattr(Both, "texts_of", lambda self, pages: [self.texts(p[0][None].numpy(), p[1][None].numpy())[0] for p in pages], raising=False)
    from bb_ocr_amd import extractor_batch

    r = Both()
    paths = list(gif_paths) + list(bmp_paths)
    want = dict(gif_want)
    want.update({len(gif_paths) + i: t for i, t in bmp_want.items()})
    assert extractor_batch.read_files(r, paths, None, 64, 4, mixed=True, **KW) == want
    assert calls_of(r, "decode_gif_pages") == [(8,)] and calls_of(r, "decode_bmp_pages") == [(7,)] and calls_of(r, "readtext_pages") == [(19,)]
