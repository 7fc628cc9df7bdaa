"""-m gpu: the device BMP decoder (bbocr_bmp_decode; csrc/bmpdec.hip) against tests/bmp_decode_ref.py byte for byte and against
``reader.decode_file``: one call that mixes every header size, depth, mask layout, direction and shape; strided destinations between guard
bytes; per-file argument errors; and the callers with ``bmp_decode=True``.  (tools/gifdec_hostcheck.py has read every byte the kernel
reads of every file here from an exact-size copy under a sanitizer on the host.)"""
import io

import numpy as np
import pytest
import torch

import bmp_decode_ref as R

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xEE
ERR_ARG = -1                                                              # bbocr.h BBOCR_ERR_ARG


@pytest.fixture(scope="module")
def good():
    """[(name, file, the restatement's decode)]: computed once, shared, never changed"""
    return [(n, f, R.decode(f)) for n, f in R.matrix() + R.handbuilt()]


def pages_of(files):
    from bb_ocr_amd import reader as M

    return [M.BmpPage(f, M.bmp_plan(f)) for f in files]


def decode_guarded(reader, files, extra=(5, 3)):
    """ONE bbocr_bmp_decode call of files of any shapes into one device buffer: per file and plane GUARD bytes, H rows at a pitch larger
    than the row, GUARD bytes.  -> (status, the buffer, [(rgb offset, rgb pitch, gray offset, gray pitch, H, W)])"""
    pages = pages_of(files)
    lay, at = [], 0
    for p in pages:
        H, W, _ = p.shape
        pr, pg = 3 * W + extra[0], W + extra[1]
        lay.append((at + GUARD, pr, at + 2 * GUARD + H * pr, pg, H, W))
        at += 3 * GUARD + H * (pr + pg)
    buf = torch.full((at,), FILL, dtype=torch.uint8, device=reader.device)
    base = buf.data_ptr()
    status = reader._bmp_decode_into(pages, [base + l[0] for l in lay], [l[1] for l in lay], [base + l[2] for l in lay], [l[3] for l in lay])
    return status, buf.cpu().numpy(), lay


def expected_buffer(size, lay, planes):
    want = np.full(size, FILL, np.uint8)
    for (o_rgb, pr, o_gray, pg, H, W), pl in zip(lay, planes):
        rows = np.arange(H)[:, None]
        want[(o_rgb + rows * pr + np.arange(3 * W)[None]).ravel()] = pl[0].ravel()
        want[(o_gray + rows * pg + np.arange(W)[None]).ravel()] = pl[1].ravel()
    return want


def test_one_call_mixes_headers_depths_layouts_and_shapes_between_guards(reader, good):
    from bb_ocr_amd.reader import decode_file

    files = [f for _, f, _ in good]
    assert {d["plan"]["bits"] for _, _, d in good} == {1, 4, 8, 16, 24, 32} and {d["plan"]["mode"] for _, _, d in good} == {0, 1, 2, 3}
    assert {d["plan"]["header_size"] for _, _, d in good} == {12, 40, 52, 56, 64, 108, 124} and len({d["rgb"].shape for _, _, d in good}) > 12
    status, buf, lay = decode_guarded(reader, files)
    assert status == [0] * len(files)
    exp = expected_buffer(buf.size, lay, [(d["rgb"], d["gray"]) for _, _, d in good])
    assert np.array_equal(buf, exp)                                       # every plane exact, guards and the bytes behind every row untouched
    for name, f, d in good[::11]:                                         # (the restatement's planes ARE decode_file's: the CPU tests; a sample here)
        rgb, gray = decode_file(f)
        assert np.array_equal(d["rgb"], rgb) and np.array_equal(d["gray"], gray), name
    status2, buf2, _ = decode_guarded(reader, files)
    assert status2 == status and np.array_equal(buf2, buf)                # two consecutive calls: identical bytes


def test_device_entry_points(reader, good):
    planes, status = reader.decode_bmp_pages(pages_of([f for _, f, _ in good[:12]]))
    assert status == [0] * 12
    for (rgb, gray), (name, _, d) in zip(planes, good):
        assert np.array_equal(rgb.cpu().numpy(), d["rgb"]) and np.array_equal(gray.cpu().numpy(), d["gray"]), name
    sources = [f for _, f, _ in good[12:30]] + [R.refusals()[-1][1], b"\xff\xd8\xff\xe0"]
    got = reader.decode_bmp_device(sources)
    assert got[-1] is None and got[-2] is None
    for g, (name, _, d) in zip(got, good[12:30]):
        assert g is not None and np.array_equal(g[0].cpu().numpy(), d["rgb"]) and np.array_equal(g[1].cpu().numpy(), d["gray"]), name
    with pytest.raises(ValueError):
        reader.decode_bmp_pages([])


def test_argument_errors_per_file(reader, good):
    f = good[4][1]
    page = pages_of([f])[0]
    H, W, _ = page.shape
    rgb = torch.full((H * W * 3 + 8,), FILL, dtype=torch.uint8, device=reader.device)
    gray = torch.full((H * W + 8,), FILL, dtype=torch.uint8, device=reader.device)
    for name, bad, _ in R.refusals():                                      # every refused file beside a good one: an argument error of its own
        refused = pages_of([f])[0]
        refused.data = bad
        assert reader._bmp_decode_into([refused, page], [rgb.data_ptr()] * 2, [3 * W] * 2, [gray.data_ptr()] * 2, [W] * 2) == [ERR_ARG, 0], name
    short = reader._bmp_decode_into([page, page, page], [rgb.data_ptr(), rgb.data_ptr(), 0], [3 * W - 1, 3 * W, 3 * W], [gray.data_ptr()] * 3, [W, W - 1, W])
    assert short == [ERR_ARG, ERR_ARG, ERR_ARG]
    assert bool((rgb[H * W * 3:] == FILL).all()) and bool((gray[H * W:] == FILL).all())
    assert np.array_equal(rgb[:H * W * 3].cpu().numpy().reshape(H, W, 3), good[4][2]["rgb"])


# ------------------------------------------------------------------------------------------------ the callers
def same_results(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x[0], np.float64), np.asarray(y[0], np.float64)) and x[1] == y[1] and x[2] == y[2]
                                    for x, y in zip(a, b))


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    """BMP pages of two shapes and every depth, JPEG pages and a BMP the plan refuses (RLE8) -> (paths, kinds)"""
    from PIL import Image

    from bb_ocr_amd import synth

    d = tmp_path_factory.mktemp("bmp_callers")
    shapes = {"A": dict(width=320, height=192, lines=3, margin=24), "B": dict(width=256, height=160, lines=2, margin=20)}
    spec = [("bmp_RGB", "A"), ("jpg", "A"), ("bmp_L", "B"), ("bmp_P", "A"), ("rle", "A"), ("bmp_1bit", "A"), ("jpg", "B"), ("bmp_RGBA", "B"),
            ("bmp_565_top_down", "A"), ("bmp_4bit", "B")]
    paths = []
    for i, (kind, shape) in enumerate(spec):
        img = synth.page(40 + i, **shapes[shape])[0]
        H, W = img.shape[:2]
        p = d / ("p%02d.%s" % (i, "jpg" if kind == "jpg" else "bmp"))
        if kind == "jpg":
            Image.fromarray(img).save(p, quality=92)
        elif kind == "rle":
            p.write_bytes(R.rle8_file(img[..., 1], R.grays(256)))         # the plan refuses it, Pillow reads it
        elif kind == "bmp_565_top_down":
            a = img.astype(np.uint16)
            px = ((a[..., 0] >> 3) << 11) | ((a[..., 1] >> 2) << 5) | (a[..., 2] >> 3)
            stride = ((W * 16 + 31) >> 3) & ~3
            rows = np.zeros((H, stride), np.uint8)
            rows[:, :2 * W] = px.astype("<u2").view(np.uint8).reshape(H, 2 * W)
            p.write_bytes(R.bmp_file(W, H, 16, pixels=rows.tobytes(), compression=3, masks=(0xF800, 0x7E0, 0x1F), top_down=True))
        elif kind == "bmp_4bit":
            idx = (img[..., 1] >> 4).astype(np.uint8)
            stride = ((W * 4 + 31) >> 3) & ~3
            rows = np.zeros((H, stride), np.uint8)
            rows[:, :W // 2] = (idx[:, 0::2] << 4) | idx[:, 1::2]
            p.write_bytes(R.bmp_file(W, H, 4, pixels=rows.tobytes(), table=[(17 * i, 17 * i, 16 * i) for i in range(16)]))
        else:
            pil = {"bmp_RGB": Image.fromarray(img), "bmp_L": Image.fromarray(img[..., 1]), "bmp_P": Image.fromarray(img).quantize(64),
                   "bmp_1bit": Image.fromarray(img[..., 1] > 128), "bmp_RGBA": Image.fromarray(np.dstack([img, img[..., :1]]))}[kind]
            p.write_bytes(R.pillow_file(pil))
        paths.append(str(p))
    return paths, [k for k, _ in spec]


def test_callers_with_the_option_on(reader, directory, monkeypatch):
    from PIL import Image

    from bb_ocr_amd import extractor_batch

    paths, kinds = directory
    assert reader.bmp_decode is False                                     # off unless asked for
    assert [bool(R.plan(open(p, "rb").read())["supported"]) for p in paths] == [k.startswith("bmp") for k in kinds]
    off = reader.readtext_files(paths, bmp_decode=False)
    assert sum(bool(r) for r in off) >= 6
    decoded = []
    real_pages = reader.decode_bmp_pages
    monkeypatch.setattr(reader, "decode_bmp_pages", lambda pages: (decoded.append(len(list(pages))), real_pages(pages))[1])
    for mixed in (False, True):
        del decoded[:]
        on = reader.readtext_files(paths, bmp_decode=True, mixed=mixed)
        assert all(same_results(a, b) for a, b in zip(on, off)), mixed
        # the seven BMP files the plan supports went through the device decoder: one call per shape group, or, mixed, one call for all
        assert sorted(decoded) == ([7] if mixed else [3, 4]), decoded
        res = extractor_batch.read_files(reader, paths, bmp_decode=True, mixed=mixed, device_decode=True)
        assert all(same_results(res[i], off[i]) for i in range(len(paths)))
        texts = extractor_batch.extract_texts(reader, paths, bmp_decode=True, mixed=mixed)
        assert texts == extractor_batch.extract_texts(reader, paths, bmp_decode=False, mixed=mixed)
    del decoded[:]
    assert extractor_batch.read_files(reader, paths, mixed=False).keys() == set(range(len(paths))) and not decoded      # the Reader's default: off
    one = [reader.readtext(p) for p in paths[:6]]
    monkeypatch.setattr(reader, "bmp_decode", True)
    del decoded[:]
    for p, want in zip(paths[:6], one):
        assert same_results(reader.readtext(p), want), p                  # readtext(path) of a BMP: the host path's result
        data = open(p, "rb").read()
        assert same_results(reader.readtext(data), reader.readtext(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))))    # bytes: the array rule
    assert sum(decoded) == 2 * sum(k.startswith("bmp") for k in kinds[:6])


def test_readtext_of_a_bmp_equals_readtext_of_its_pixels(reader, directory, monkeypatch):
    from bb_ocr_amd.reader import decode_file

    paths, kinds = directory
    monkeypatch.setattr(reader, "bmp_decode", True)
    for p, kind in zip(paths, kinds):
        if kind in ("bmp_RGB", "bmp_P", "bmp_RGBA", "bmp_565_top_down", "bmp_4bit"):     # colour pages: an array's gray plane is derived from its colours
            rgb, _ = decode_file(p)
            assert same_results(reader.readtext(open(p, "rb").read()), reader.readtext(rgb)), p
