"""-m gpu: the device GIF decoder (bbocr_gif_decode, bbocr_op_gif_decode_stage; csrc/gifdec.hip) against tests/gif_decode_ref.py byte for
byte -- the piece table, the offsets and the total, the index stream, both planes -- and against ``reader.decode_file``; one call that
mixes shapes, piece counts and code sizes; strided destinations between guard bytes; the status of damaged files beside good ones; and the
callers with ``gif_decode=True``.  Every file of the good list must end in status 0: none may reach its result through the host
fallback.  (tools/gifdec_hostcheck.py has run every file here through the same scan and piece walks under a sanitizer on the host; a
damaged file is an input the decoder answers with a status.)"""
import io

import numpy as np
import pytest
import torch

import gif_decode_ref as R

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xEE
ERR_ARG, ERR_DATA = -1, -7                                                # bbocr.h BBOCR_ERR_*


@pytest.fixture(scope="module")
def good():
    """[(name, file, the restatement's decode)]: Pillow's matrix, the hand-built files, the hand-written streams: computed once, shared,
    never changed"""
    return [(n, f, R.decode(f)) for n, f in R.matrix() + R.handbuilt() + R.handwritten_files()]


def pages_of(files):
    from bb_ocr_amd import reader as M

    return [M.GifPage(f, M.gif_plan(f)) for f in files]


def decode_guarded(reader, files, extra=(5, 3)):
    """ONE bbocr_gif_decode call of files of any shapes into one device buffer: per file and plane GUARD bytes, H rows at a pitch larger
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
    status = reader._gif_decode_into(pages, [base + l[0] for l in lay], [l[1] for l in lay], [base + l[2] for l in lay], [l[3] for l in lay])
    return status, buf.cpu().numpy(), lay


def expected_buffer(size, lay, planes):
    """the buffer decode_guarded must leave: FILL everywhere but in the rows' pixels; planes[k] None: that file's region is not compared"""
    want = np.full(size, FILL, np.uint8)
    mask = np.ones(size, bool)
    for (o_rgb, pr, o_gray, pg, H, W), pl in zip(lay, planes):
        rows = np.arange(H)[:, None]
        i_rgb, i_gray = (o_rgb + rows * pr + np.arange(3 * W)[None]).ravel(), (o_gray + rows * pg + np.arange(W)[None]).ravel()
        if pl is None:
            mask[i_rgb] = mask[i_gray] = False
        else:
            want[i_rgb], want[i_gray] = pl[0].ravel(), pl[1].ravel()
    return want, mask


def test_stages_equal_the_restatement(reader, good):
    for name, f, d in good:
        s0, st = reader.gif_decode_stage(f, 0)
        assert st == 0 and s0 == d["stage0"], name
        s1, st = reader.gif_decode_stage(f, 1)
        assert st == 0 and s1 == d["stage1"], name
        s2, st = reader.gif_decode_stage(f, 2)
        assert st == 0 and s2 == d["stage2"], name


def test_stage_arguments(reader, good):
    import ctypes as C

    f = good[0][1]                                                        # 96x64, 3 pieces
    pl = R.plan(f)
    room = R.piece_cap(pl["payload_bytes"], pl["min_code"])
    dst = torch.zeros(16 + 16 * room, dtype=torch.uint8, device=reader.device)
    st = C.c_int()
    call = lambda data, stage, n: reader._lib.bbocr_op_gif_decode_stage(reader._h, data, len(data), stage, C.c_void_p(dst.data_ptr()), n, C.byref(st))
    assert call(f, 0, 16 + 16 * room) == 0 and call(f, 0, 15 + 16 * room) == ERR_ARG and call(f, 3, 16 + 16 * room) == ERR_ARG
    assert call(f, 1, 4 * room + 4) == 0 and call(f, 1, 4 * room + 3) == ERR_ARG
    assert call(f, 2, 96 * 64) == 0 and call(f, 2, 96 * 64 - 1) == ERR_ARG and call(R.refusals()[-1][1], 0, 16 + 16 * room) == ERR_ARG


def test_one_call_mixes_shapes_pieces_and_code_sizes_between_guards(reader, good):
    """the full call against the restatement (whose planes ARE decode_file's: the CPU tests; a sample here): every good file in ONE
    batch, into strided destinations whose guard bytes and row tails must stay untouched"""
    from bb_ocr_amd.reader import decode_file

    files = [f for _, f, _ in good]
    assert {d["plan"]["min_code"] for _, _, d in good} == set(range(2, 9)) and len({d["rgb"].shape for _, _, d in good}) > 12
    assert {1, 2, 3, 5, 92} <= {len(d["stages"]["pieces"]) for _, _, d in good}
    status, buf, lay = decode_guarded(reader, files)
    assert status == [0] * len(files)                                     # no file reaches its result through the host fallback
    exp, _ = expected_buffer(buf.size, lay, [(d["rgb"], d["gray"]) for _, _, d in good])
    assert np.array_equal(buf, exp)                                       # every plane exact, guards and the bytes behind every row untouched
    for name, f, d in good[::7]:
        rgb, gray = decode_file(f)
        assert np.array_equal(d["rgb"], rgb) and np.array_equal(d["gray"], gray), name
    status2, buf2, _ = decode_guarded(reader, files)
    assert status2 == status and np.array_equal(buf2, buf)                # two consecutive calls: identical bytes


def test_device_entry_points(reader, good):
    planes, status = reader.decode_gif_pages(pages_of([f for _, f, _ in good[:9]]))
    assert status == [0] * 9
    for (rgb, gray), (name, _, d) in zip(planes, good):
        assert np.array_equal(rgb.cpu().numpy(), d["rgb"]) and np.array_equal(gray.cpu().numpy(), d["gray"]), name
    sources = [f for _, f, _ in good[9:20]] + [R.refusals()[-1][1], b"\xff\xd8\xff\xe0"]
    got = reader.decode_gif_device(sources)
    assert got[-1] is None and got[-2] is None
    for g, (name, _, d) in zip(got, good[9:20]):
        assert g is not None and np.array_equal(g[0].cpu().numpy(), d["rgb"]) and np.array_equal(g[1].cpu().numpy(), d["gray"]), name


def test_damaged_files_beside_good_ones(reader, good):
    bad = R.damaged()
    pick = good[1::9][:len(bad) + 1]
    assert len(pick) == len(bad) + 1
    files, planes, is_bad = [], [], []
    for k, (_, f, d) in enumerate(pick):                                  # good, bad, good, bad, ... good
        files.append(f)
        planes.append((d["rgb"], d["gray"]))
        is_bad.append(False)
        if k < len(bad):
            files.append(bad[k][1])
            planes.append(None)
            is_bad.append(True)
    status, buf, lay = decode_guarded(reader, files)
    assert [s != 0 for s in status] == is_bad and all(s in (0, ERR_DATA) for s in status), list(zip(status, is_bad))
    exp, mask = expected_buffer(buf.size, lay, planes)
    assert np.array_equal(buf[mask], exp[mask])                           # the good files exact; no byte outside any destination's rows
    for name, f in bad:                                                   # ... and each alone, through the entry points of the callers
        assert reader.decode_gif_device([f]) == [None], name
        assert reader.gif_decode_stage(f, 2)[1] == ERR_DATA, name
        assert reader.gif_decode_stage(f, 0)[0] == R.decode(f)["stage0"], name       # the scan itself is sound
    status, buf, lay = decode_guarded(reader, [f for _, f, _ in pick])    # the context serves a further call
    assert status == [0] * len(pick)
    assert np.array_equal(buf, expected_buffer(buf.size, lay, [(d["rgb"], d["gray"]) for _, _, d in pick])[0])


def test_piece_table_overflow_is_a_status(reader, good):
    """more pieces than the table's room: a status of that file, never a silent truncation; its neighbour decodes"""
    m, n = 2, 4200
    pay = R.pack_codes([c for b in R.noisy(n, 1, m, seed=1) for c in (4, b)] + [5], m)
    f = R.gif_file(70, 60, m, pay, gct=R.colours(4, 1))
    status, buf, lay = decode_guarded(reader, [f, good[0][1]])
    assert status == [ERR_DATA, 0]
    exp, mask = expected_buffer(buf.size, lay, [None, (good[0][2]["rgb"], good[0][2]["gray"])])
    assert np.array_equal(buf[mask], exp[mask])
    head = np.frombuffer(reader.gif_decode_stage(f, 0)[0][:16], np.uint32)
    assert list(head) == [4096, R.ERR_PIECES, 0, 0]


def test_argument_errors_per_file(reader, good):
    f = good[5][1]
    page = pages_of([f])[0]
    H, W, _ = page.shape
    rgb = torch.full((H * W * 3 + 8,), FILL, dtype=torch.uint8, device=reader.device)
    gray = torch.full((H * W + 8,), FILL, dtype=torch.uint8, device=reader.device)
    refused = pages_of([f])[0]
    refused.data = R.refusals()[-1][1]
    short = reader._gif_decode_into([page, page, refused, page], [rgb.data_ptr()] * 4, [3 * W - 1, 3 * W, 3 * W, 3 * W], [gray.data_ptr()] * 4, [W, W - 1, W, W])
    assert short == [ERR_ARG, ERR_ARG, ERR_ARG, 0]
    assert bool((rgb[H * W * 3:] == FILL).all()) and bool((gray[H * W:] == FILL).all())
    assert reader._gif_decode_into([page], [0], [3 * W], [gray.data_ptr()], [W]) == [ERR_ARG]


# ------------------------------------------------------------------------------------------------ the callers
def same_results(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x[0], np.float64), np.asarray(y[0], np.float64)) and x[1] == y[1] and x[2] == y[2]
                                    for x, y in zip(a, b))


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    """GIF pages of two shapes (gray, palette, interlaced), JPEG pages, a GIF the plan refuses (no terminator) and a GIF whose stream is cut
    -> (paths, kinds)"""
    from PIL import Image

    from bb_ocr_amd import synth

    d = tmp_path_factory.mktemp("gif_callers")
    shapes = {"A": dict(width=320, height=192, lines=3, margin=24), "B": dict(width=256, height=160, lines=2, margin=20)}
    spec = [("gif_L", "A"), ("jpg", "A"), ("gif_P", "B"), ("gif_P_interlaced", "A"), ("refused", "A"), ("gif_1bit", "A"), ("jpg", "B"),
            ("gif_L", "B"), ("cut", "A"), ("gif_P", "A")]
    paths = []
    for i, (kind, shape) in enumerate(spec):
        img = synth.page(40 + i, **shapes[shape])[0]
        p = d / ("p%02d.%s" % (i, "jpg" if kind == "jpg" else "gif"))
        if kind == "jpg":
            Image.fromarray(img).save(p, quality=92)
            paths.append(str(p))
            continue
        pil = Image.fromarray(img[..., 1] > 128) if kind == "gif_1bit" else (Image.fromarray(img) if "_P" in kind else Image.fromarray(img[..., 1]))
        f = R.pillow_file(pil, interlace=int(kind.endswith("interlaced")))
        if kind == "refused":
            f = f[:-2]                                                    # neither the terminator nor the trailer: Pillow reads it, the plan does not
        elif kind == "cut":
            pl = R.plan(f)
            f = R.gif_file(pl["width"], pl["height"], pl["min_code"], pl["payload"][:pl["payload_bytes"] // 2], gct=pl["table"])
        p.write_bytes(f)
        paths.append(str(p))
    return paths, [k for k, _ in spec]


def test_callers_with_the_option_on(reader, directory, monkeypatch):
    from PIL import Image

    from bb_ocr_amd import extractor_batch

    paths, kinds = directory
    assert reader.gif_decode is False                                     # off unless asked for
    assert [bool(R.plan(open(p, "rb").read())["supported"]) for p in paths] == [k.startswith("gif") or k == "cut" for k in kinds]
    off = reader.readtext_files(paths, gif_decode=False)
    assert sum(bool(r) for r in off) >= 7
    decoded = []
    real_pages = reader.decode_gif_pages
    monkeypatch.setattr(reader, "decode_gif_pages", lambda pages: (decoded.append(len(list(pages))), real_pages(pages))[1])
    for mixed in (False, True):
        del decoded[:]
        on = reader.readtext_files(paths, gif_decode=True, mixed=mixed)
        assert all(same_results(a, b) for a, b in zip(on, off)), mixed
        # the seven GIF files the plan supports (the cut one among them) went through the device decoder: one call per shape group, or,
        # mixed, one call for all of them
        assert sorted(decoded) == ([7] if mixed else [2, 5]), decoded
        res = extractor_batch.read_files(reader, paths, gif_decode=True, mixed=mixed, device_decode=True)
        assert all(same_results(res[i], off[i]) for i in range(len(paths)))
        texts = extractor_batch.extract_texts(reader, paths, gif_decode=True, mixed=mixed)
        assert texts == extractor_batch.extract_texts(reader, paths, gif_decode=False, mixed=mixed)
    del decoded[:]
    assert extractor_batch.read_files(reader, paths, mixed=False).keys() == set(range(len(paths))) and not decoded      # the Reader's default: off
    one = [reader.readtext(p) for p in paths[:6]]
    monkeypatch.setattr(reader, "gif_decode", True)
    del decoded[:]
    for p, want in zip(paths[:6], one):
        assert same_results(reader.readtext(p), want), p                  # readtext(path) of a GIF: the host path's result
        data = open(p, "rb").read()
        assert same_results(reader.readtext(data), reader.readtext(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))))    # bytes: the array rule
    assert sum(decoded) == 2 * sum(k.startswith("gif") for k in kinds[:6])


def test_readtext_of_a_gif_equals_readtext_of_its_pixels(reader, directory, monkeypatch):
    from bb_ocr_amd.reader import decode_file

    paths, kinds = directory
    monkeypatch.setattr(reader, "gif_decode", True)
    for p, kind in zip(paths, kinds):
        if kind.startswith("gif_P"):                                      # palette pages: an array's gray plane is derived from its colours
            rgb, _ = decode_file(p)
            assert same_results(reader.readtext(open(p, "rb").read()), reader.readtext(rgb)), p
