"""f3 without a card: what ``extractor_batch.read_files`` asks of its Reader, per page kind -- the uploaded batch, the failed upload, the
batch whose device call fails, and the ``"jpg"`` groups of ``device_decode=True`` with their per-file status.  A recording double stands
in for the Reader (Pillow, numpy and CPU torch only; ``jpeg_plan`` needs the built library, as in test_jpeg_decode_cpu.py).  Every case
must return what reading the files one by one returns, and make exactly the calls listed."""
import collections
import io
import zlib

import numpy as np
import pytest
import torch

from oracle import imgproc

A, B, C = (48, 64), (300, 400), (150, 200)                                # page shapes (H, W)
MAX_BATCH, WORKERS = 4, 8
# 37 files: (file kind, shape).  The kinds a file travels as: "png" / "pngL" / "jpgL" -> "rgb", "jpg" / "prog" -> "ycc"; with
# device_decode=True "jpg" -> "jpg" [n,H,W,4], "jpgL" -> "jpg" [n,H,W], and the progressive file, which the plan refuses, stays "ycc"
SPEC = [("png", A)] * 7 + [("png", B)] * 5 + [("pngL", A)] * 5 + [("jpg", B)] * 9 + [("jpg", C)] * 9 + [("jpgL", C), ("prog", B)]
HOST_KIND = {"png": "rgb", "pngL": "rgb", "jpgL": "rgb", "jpg": "ycc", "prog": "ycc"}
DEVICE_KIND = {"png": "rgb", "pngL": "rgb", "jpgL": "jpgL", "jpg": "jpg", "prog": "ycc"}
POISON = (1, 2, 3)                                                        # pixel [0,0] of one ("png", B) page
KW = {"min_size": 7}                                                      # readtext keywords: handed to every read call unchanged


class FakeReader:
    """The page-by-page double of test_abi_host_cpu.py: host pages in, per page a text that is a function of both planes; a batch holding
    the poison page fails as a whole.  Every call is recorded as (name, shape of its batch)."""

    def __init__(self, poison=None):
        self.poison, self.calls = poison, []

    def _note(self, name, shape, kw=KW):
        assert kw == KW
        self.calls.append((name, tuple(int(v) for v in shape)))

    def texts(self, rgb, gray):
        assert rgb.shape[:3] == gray.shape and rgb.shape[3] == 3 and rgb.dtype == gray.dtype == np.uint8
        if any(tuple(p[0, 0].tolist()) == self.poison for p in rgb):
            raise RuntimeError("boom")
        return [[(None, f"w{p.shape[1]}", 0.9), (None, "%08x" % zlib.crc32(g.tobytes(), zlib.crc32(p.tobytes())), 0.5)] for p, g in zip(rgb, gray)]

    def readtext_arrays(self, rgb, gray=None, **kw):
        rgb, gray = np.stack(rgb), np.stack(gray)                         # the batching loop hands over LISTS of equal-shape pages
        self._note("readtext_arrays", rgb.shape, kw)
        return self.texts(rgb, gray)

    def readtext_ycc_arrays(self, ycc, **kw):
        ycc = np.stack(ycc)                                               # 3 or 4 bytes per pixel
        self._note("readtext_ycc_arrays", ycc.shape, kw)
        return self.texts(imgproc.jpeg_ycc_to_rgb(ycc[..., :3]), np.ascontiguousarray(ycc[..., 0]))


class FakeDeviceReader(FakeReader):
    """... with the device entries ``read_files`` uses (CPU tensors stand for device memory) and switches that make them fail:
    ``fail_to_dev`` / ``fail_decode``: the call raises; ``fail_device(rgb)``: ``readtext_device`` raises where it returns True;
    ``bad_files``: file bytes whose decode status is non-zero (their page of the batch is zeroed: it must not be read)."""

    def __init__(self, poison=None, fail_to_dev=False, fail_decode=False, fail_device=None, bad_files=()):
        super().__init__(poison)
        self.fail_to_dev, self.fail_decode, self.fail_device, self.bad_files = fail_to_dev, fail_decode, fail_device, set(bad_files)

    def _to_dev(self, arr):
        assert isinstance(arr, list)
        self._note("_to_dev", (len(arr),) + arr[0].shape)
        if self.fail_to_dev:
            raise RuntimeError("upload failed")
        return torch.from_numpy(np.stack(arr))

    def pages_from_ycc(self, ycc):
        self._note("pages_from_ycc", ycc.shape)
        a = ycc.numpy()
        return torch.from_numpy(imgproc.jpeg_ycc_to_rgb(a[..., :3])), torch.from_numpy(np.ascontiguousarray(a[..., 0]))

    def readtext_device(self, rgb, gray=None, **kw):
        self._note("readtext_device", rgb.shape, kw)
        assert rgb.is_contiguous() and gray.is_contiguous()
        if self.fail_device is not None and self.fail_device(rgb):
            raise RuntimeError("device call failed")
        return self.texts(rgb.numpy(), gray.numpy())

    def decode_jpeg_batch(self, pages, padded=False):
        from PIL import Image

        pages = list(pages)
        assert padded and all(p.shape == pages[0].shape for p in pages)
        self._note("decode_jpeg_batch", (len(pages),) + pages[0].shape)
        if self.fail_decode:
            raise RuntimeError("decode failed")
        out = []
        for p in pages:
            pil = Image.open(io.BytesIO(p.data))
            if p.shape[2] == 3:
                pil.draft("YCbCr", pil.size)
                a = np.asarray(pil)
                a = np.concatenate([a, np.full_like(a[..., :1], 255)], axis=2)
            else:
                a = np.asarray(pil)
            assert a.shape[:2] == p.shape[:2]
            out.append(np.zeros_like(a) if p.data in self.bad_files else a)
        return torch.from_numpy(np.stack(out)), [(-3 if p.data in self.bad_files else 0) for p in pages]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(paths, want): the 37 files in a fixed shuffled order, and per index the result of reading that file alone"""
    from PIL import Image

    from bb_ocr_amd.reader import decode_file

    d = tmp_path_factory.mktemp("read_files")
    rng = np.random.default_rng(5)
    order = rng.permutation(len(SPEC)).tolist()
    spec = [SPEC[k] for k in order]
    paths, poisoned = [], False
    for i, (kind, (h, w)) in enumerate(spec):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        a[0, 0] = (9, 9, 9)
        if (kind, (h, w)) == ("png", B) and not poisoned:
            a[0, 0], poisoned = POISON, True
        p = d / f"p{i:02d}.{'png' if kind.startswith('png') else 'jpg'}"
        if kind == "png":
            Image.fromarray(a).save(p)
        elif kind == "pngL":
            Image.fromarray(a[..., 0]).save(p)
        elif kind == "jpgL":
            Image.fromarray(a[..., 0]).save(p, quality=90)
        else:
            Image.fromarray(a).save(p, quality=90, progressive=(kind == "prog"))       # Pillow's default: 4:2:0
        paths.append(p)
    ref = FakeReader()
    want = {i: ref.texts(*[x[None] for x in decode_file(p)])[0] for i, p in enumerate(paths)}
    return paths, spec, want


def batches(spec, kinds, skip=()):
    """The batches ``read_files`` forms: pages are grouped by (kind, shape) in file order, and a group travels when it holds MAX_BATCH pages
    or at the end.  (The window is 2 * WORKERS = 16 pages and at most 14 can wait in partial groups -- three in each of four groups and the
    two single files -- so no group is sent early for want of a slot.)  -> [(kind, [file index, ...])]"""
    groups = collections.OrderedDict()
    for i, (kind, shape) in enumerate(spec):
        if i not in skip:
            groups.setdefault((kinds[kind], shape), []).append(i)
    return [(key[0], idx[k:k + MAX_BATCH]) for key, idx in groups.items() for k in range(0, len(idx), MAX_BATCH)]


def uploaded_calls(kind, n):
    """the calls of one uploaded batch whose device call succeeds"""
    return {"rgb": [("_to_dev", n)] * 2 + [("readtext_device", n)],
            "ycc": [("_to_dev", n), ("pages_from_ycc", n), ("readtext_device", n)],
            "jpg": [("decode_jpeg_batch", n), ("pages_from_ycc", n), ("readtext_device", n)],
            "jpgL": [("decode_jpeg_batch", n), ("readtext_device", n)]}[kind]


HOST_PAGE = {"rgb": "readtext_arrays", "ycc": "readtext_ycc_arrays", "jpg": "readtext_ycc_arrays", "jpgL": "readtext_arrays"}


def made(reader):
    return collections.Counter((name, shape[0]) for name, shape in reader.calls)


def run(reader, paths, **kw):
    from bb_ocr_amd.extractor_batch import read_files

    return read_files(reader, paths, None, MAX_BATCH, WORKERS, **kw, **KW)


def poison_index(spec, paths):
    return next(i for i, s in enumerate(spec) if s == ("png", B))         # the first such file carries the pixel


def test_host_reader_without_upload_entry(files):
    paths, spec, want = files
    fr = FakeReader()
    assert run(fr, paths) == want
    assert made(fr) == collections.Counter((HOST_PAGE[k], len(idx)) for k, idx in batches(spec, HOST_KIND))


def test_uploaded_batches(files):
    paths, spec, want = files
    fd = FakeDeviceReader()
    assert run(fd, paths) == want
    groups = batches(spec, HOST_KIND)
    assert made(fd) == collections.Counter(c for k, idx in groups for c in uploaded_calls(k, len(idx)))
    assert not any(name in ("readtext_arrays", "readtext_ycc_arrays") for name, _ in fd.calls)
    # a ycc group goes through pages_from_ycc as uploaded (3 or 4 bytes per pixel), an rgb group never
    ycc_shapes = sorted(s[:3] for name, s in fd.calls if name == "pages_from_ycc")
    assert ycc_shapes == sorted((len(idx),) + spec[idx[0]][1] for k, idx in groups if k == "ycc")


def test_upload_fails(files):
    paths, spec, want = files
    fd = FakeDeviceReader(fail_to_dev=True)
    assert run(fd, paths) == want
    # one upload attempt per batch, then the batch is read from the host lists
    assert made(fd) == collections.Counter(c for k, idx in batches(spec, HOST_KIND) for c in [("_to_dev", len(idx)), (HOST_PAGE[k], len(idx))])


def test_device_call_fails_for_the_batch_with_the_poison_page(files):
    paths, spec, want = files
    bad = poison_index(spec, paths)
    fd = FakeDeviceReader(poison=POISON)
    assert run(fd, paths) == {**want, bad: []}
    exp = collections.Counter()
    for k, idx in batches(spec, HOST_KIND):
        exp.update(uploaded_calls(k, len(idx)))
        if bad in idx:                                  # the host lists as one batch, then page by page: only the poison page is lost
            exp.update([("readtext_arrays", len(idx))] + [("readtext_arrays", 1)] * len(idx))
    assert made(fd) == exp
    fr = FakeReader(poison=POISON)                      # the same without the upload stage
    assert run(fr, paths) == {**want, bad: []}


def test_device_decode_groups(files):
    from bb_ocr_amd.extractor_batch import extract_texts

    paths, spec, want = files
    fd = FakeDeviceReader()
    assert run(fd, paths, device_decode=True) == want
    groups = batches(spec, DEVICE_KIND)
    assert sorted(len(idx) for k, idx in groups if k == "jpg") == [1, 1, 4, 4, 4, 4] and [len(idx) for k, idx in groups if k == "jpgL"] == [1]
    assert made(fd) == collections.Counter(c for k, idx in groups for c in uploaded_calls(k, len(idx)))
    # grouped by decoded shape, one decode call per group; the grey file is a group of its own, [n,H,W]
    assert sorted(s for name, s in fd.calls if name == "decode_jpeg_batch") == sorted((len(idx),) + spec[idx[0]][1] + ((3,) if k == "jpg" else (1,))
                                                                                      for k, idx in groups if k in ("jpg", "jpgL"))
    # ... whose RGB is the plane replicated: its text is that of decode_file's (rgb, gray), and no pages_from_ycc call was made for it
    grey = next(i for i, s in enumerate(spec) if s[0] == "jpgL")
    plane = _grey_plane(paths[grey])
    assert want[grey] == FakeReader().texts(np.repeat(plane[None, :, :, None], 3, axis=3), plane[None])[0]
    # the extractor's decode step (no file here is above the limit) makes the same groups
    fx = FakeDeviceReader()
    assert extract_texts(fx, paths, None, MAX_BATCH, WORKERS, device_decode=True, **KW) == {i: " ".join(t[1] for t in r) for i, r in want.items()}
    assert made(fx) == made(fd)


def _grey_plane(path):
    from PIL import Image

    return np.asarray(Image.open(path).convert("L"))


def _jpg_expectation(groups, failed):
    """calls when the jpg batches ``failed`` maps to a list of calls take those instead of the successful ones"""
    return collections.Counter(c for n, (k, idx) in enumerate(groups) for c in (failed[n] if n in failed else uploaded_calls(k, len(idx))))


def test_device_decode_status(files):
    paths, spec, want = files
    groups = batches(spec, DEVICE_KIND)
    n4 = next(n for n, (k, idx) in enumerate(groups) if k == "jpg" and len(idx) == 4)
    nl = next(n for n, (k, idx) in enumerate(groups) if k == "jpgL")
    bad = [groups[n4][1][1], groups[nl][1][0]]          # one file among three good neighbours, and the grey file (a group of one)
    fd = FakeDeviceReader(bad_files=[open(paths[i], "rb").read() for i in bad])
    assert run(fd, paths, device_decode=True) == want
    # the neighbours stay on the device; the two files take the host decode, one page per call
    assert made(fd) == _jpg_expectation(groups, {
        n4: [("decode_jpeg_batch", 4), ("pages_from_ycc", 3), ("readtext_device", 3), ("readtext_ycc_arrays", 1)],
        nl: [("decode_jpeg_batch", 1), ("readtext_arrays", 1)]})


def test_device_decode_call_fails(files):
    paths, spec, want = files
    groups = batches(spec, DEVICE_KIND)
    fd = FakeDeviceReader(fail_decode=True)
    assert run(fd, paths, device_decode=True) == want
    assert made(fd) == _jpg_expectation(groups, {n: [("decode_jpeg_batch", len(idx))] + [(HOST_PAGE[k], 1)] * len(idx)
                                                 for n, (k, idx) in enumerate(groups) if k in ("jpg", "jpgL")})


def test_device_call_fails_on_jpg_groups(files):
    paths, spec, want = files
    groups = batches(spec, DEVICE_KIND)
    fd = FakeDeviceReader(fail_device=lambda rgb: tuple(rgb.shape[1:3]) == C)       # the colour groups of shape C and the grey file
    assert run(fd, paths, device_decode=True) == want
    failed = {n: uploaded_calls(k, len(idx)) + [(HOST_PAGE[k], 1)] * len(idx)
              for n, (k, idx) in enumerate(groups) if k in ("jpg", "jpgL") and spec[idx[0]][1] == C}
    assert len(failed) == 4
    assert made(fd) == _jpg_expectation(groups, failed)


def test_decode_callback_that_fails(files):
    from bb_ocr_amd.extractor_batch import _plain_input, read_files

    paths, spec, want = files

    def decode(path, i):
        if i == 3:
            raise RuntimeError("unreadable")
        return None if i == 11 else _plain_input(path, i)

    fd = FakeDeviceReader()
    got = read_files(fd, paths, None, MAX_BATCH, WORKERS, decode=decode, **KW)
    assert got == {**want, 3: [], 11: []}
    # every other index exactly once
    assert made(fd) == collections.Counter(c for k, idx in batches(spec, HOST_KIND, skip=(3, 11)) for c in uploaded_calls(k, len(idx)))
    assert sum(n for (name, n), c in made(fd).items() for _ in range(c) if name == "readtext_device") == len(paths) - 2


def test_ocr_input_page_kinds(tmp_path):
    """the decode steps of extract_texts: which kind a file becomes, and that every kind holds ``ocr_input_image``'s pixels"""
    from PIL import Image

    from bb_ocr_amd import extractor_batch as eb

    rng = np.random.default_rng(2)
    big = tmp_path / "big.png"
    Image.fromarray(rng.integers(0, 256, (120, 1700, 3), dtype=np.uint8)).save(big)
    jpg = tmp_path / "small.jpg"
    Image.fromarray(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)).save(jpg, quality=90)
    rgb, gray = eb.ocr_input_image(big, 0)
    assert rgb.shape == (113, 1600, 3)
    kind, ycc, none = eb._ocr_input(big, 0)
    assert kind == "ycc" and none is None and np.array_equal(imgproc.jpeg_ycc_to_rgb(ycc[..., :3]), rgb) and np.array_equal(ycc[..., 0], gray)
    kind, a, g = eb._ocr_input(big, 0, decode_once=False)
    assert kind == "rgb" and np.array_equal(a, rgb) and np.array_equal(g, gray)
    kind, page, none = eb._ocr_input(big, 0, device_decode=True)              # the thumbnail as written travels as its bytes
    assert kind == "jpg" and none is None and page.shape == rgb.shape
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(page.data)).convert("RGB")), rgb)
    kind, a, g = eb._ocr_input(big, 3, device_decode=True)                    # below 2400: the PNG itself
    assert kind == "rgb" and a.shape == (120, 1700, 3) and np.array_equal(a, np.asarray(Image.open(big)))
    kind, page, none = eb._ocr_input(jpg, 0, device_decode=True)
    assert kind == "jpg" and page.data == open(jpg, "rb").read() and page.shape == (48, 64, 3)
    assert eb._ocr_input(jpg, 0)[0] == "ycc" and eb._ocr_input(jpg, 0, decode_once=False)[0] == "rgb"
    assert [eb._plain_input(p)[0] for p in (big, jpg)] == ["rgb", "ycc"] and [eb._plain_input_device(p)[0] for p in (big, jpg)] == ["rgb", "jpg"]
    with pytest.raises(Exception):
        eb._ocr_input(tmp_path / "missing.png", 0)
    # a page held as an array (the cropped page): thumbnailed like the file the reference writes
    page = rng.integers(0, 256, (120, 1700), dtype=np.uint8)
    kind, ycc, none = eb._ocr_input_array(page, 0)
    k2, a, g = eb._ocr_input_array(page, 0, decode_once=False)
    assert (kind, k2) == ("ycc", "rgb") and np.array_equal(imgproc.jpeg_ycc_to_rgb(ycc[..., :3]), a) and np.array_equal(ycc[..., 0], g)
    kind, a, g = eb._ocr_input_array(page, 3)
    assert kind == "rgb" and np.array_equal(g, page) and np.array_equal(a, np.repeat(page[:, :, None], 3, 2))
