"""The device GIF decoder without a card: the restatement (tests/gif_decode_ref.py) against ``reader.decode_file`` (Pillow plus the stated
gray rule) over Pillow's own files, the hand-built files and the hand-written code streams; the split at the clear codes against one serial
walk; ``bbocr_host_gif_plan`` through ctypes against the restatement's walk -- every field, the table, every refusal reason --; the damage
list against Pillow; the classes that are stricter than Pillow; the ABI exports."""
import ctypes as C
import io
import warnings

import numpy as np
import pytest

import gif_decode_ref as R


@pytest.fixture(scope="module")
def good():
    return [(n, f, R.decode(f)) for n, f in R.matrix() + R.handbuilt() + R.handwritten_files()]


def host_decode(f):
    from bb_ocr_amd.reader import decode_file

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return decode_file(f)


def lib_plan(f):
    from bb_ocr_amd.reader import gif_plan

    p = gif_plan(f)
    return {k: int(getattr(p, k)) for k in R.PLAN_FIELDS}, bytes(p.table)


def test_restatement_equals_decode_file(good):
    from PIL import Image

    modes = set()
    for name, f, d in good:
        rgb, gray = host_decode(f)
        assert d["status"] == 0 and np.array_equal(d["rgb"], rgb) and np.array_equal(d["gray"], gray), name
        mode = Image.open(io.BytesIO(f)).mode
        assert (mode == "L") == bool(d["plan"]["mode_l"]) and mode in ("L", "P"), name
        modes.add((mode, d["plan"]["interlace"]))
    assert modes == {("L", 0), ("L", 1), ("P", 0), ("P", 1)}
    tables = {d["plan"]["table_len"] for n, _, d in good if n.startswith("modeP_")}
    assert tables == {4, 8, 16, 64, 128, 256}                                     # Pillow rounds 2, 3, 7, 33 and 200 colours up
    assert {d["plan"]["table_len"] for _, _, d in good} == {0, 2, 4, 8, 16, 32, 64, 128, 256}


def test_pieces_equal_one_serial_walk(good):
    """the split at the clear codes -- closed-form positions, pieces decoded on their own, offsets from the lengths -- gives what one
    serial walk with incremental widths gives"""
    for name, f, d in good:
        pl, st = d["plan"], d["stages"]
        need = pl["width"] * pl["height"]
        assert R.serial_indices(pl["payload"], pl["min_code"], need) == d["stage2"], name
        assert st["total"] == need and st["offsets"] == [min(sum(st["lengths"][:i]), need) for i in range(len(st["pieces"]))], name
    for m in range(2, 9):                                                          # the closed form against the sum of the widths
        pos = 0
        for k in range(5000):
            assert R.code_pos(m, k) == pos, (m, k)
            pos += R.code_width(m, k)
        assert R.code_width(m, 0) == m + 1 and R.code_width(m, 4094 - (1 << m)) == 12 == R.code_width(m, 10 ** 6)


def test_sizes_and_piece_counts_the_device_tests_rely_on(good):
    by = {n: d for n, _, d in good}
    pieces = lambda n: len(by[n]["stages"]["pieces"])
    assert pieces("noisy_L_96x64") == 3 and pieces("noisy_L_128x96") == 5           # Pillow clears after every 3,839 data codes
    assert [c for _, c, _ in by["noisy_L_128x96"]["stages"]["pieces"][:3]] == [0, 3839, 3839]
    assert by["one_pixel"]["rgb"].shape == (1, 1, 3) and by["one_by_n"]["rgb"].shape == (41, 1, 3) and by["n_by_one"]["rgb"].shape == (1, 41, 3)
    assert by["interlaced_9_rows"]["plan"]["interlace"] == 1 and by["interlaced_17_rows"]["plan"]["height"] == 17
    assert max(d["rgb"].shape[0] * d["rgb"].shape[1] for d in by.values()) <= 256 * 192
    assert by["frame_past_tNone_i0"]["rgb"].shape == (7, 9, 3)                     # a 6x5 frame at (3,2) on a 4x4 screen


def test_handwritten_streams_hold_what_their_names_say():
    by = {n: (w, h, m, pay) for n, w, h, m, pay in R.handwritten()}
    assert sorted(m for n, _, _, m, _ in R.handwritten() if n[0] == "m" and n[1:].isdigit()) == list(range(2, 9))
    scan = lambda n: R.scan(by[n][3], by[n][2])[0]
    w, h, m, pay = by["clear_before_every_code"]
    assert [(c, e) for _, c, e in scan("clear_before_every_code")] == [(0, R.END_CLEAR)] + [(1, R.END_CLEAR)] * (w * h - 1) + [(1, R.END_EOI)]
    assert [c for _, c, _ in scan("two_clears_in_a_row")][:2] == [0, 0] and [c for _, c, _ in scan("two_clears_in_a_row")].count(0) == 4
    assert scan("no_leading_clear")[0][1] > 0 and len(scan("no_leading_clear")) == 1
    never = scan("never_clears")
    # one piece that runs on at 12 bits with the table full for thousands of codes: dozens of 64-code scan steps in that regime
    assert [c > 4096 - 258 + 64 * 40 for _, c, _ in never] == [False, True] and never[1][2] == R.END_EOI
    for at in (63, 64, 65, 127, 128):                                              # the clear as lane 63 of a step, lane 0 of the next, ...
        assert [c for _, c, _ in scan("clear_at_%d" % at)][1:3] == [at, at]
    assert R.code_width(6, 62) == 7 and R.code_width(6, 63) == 8 and R.code_width(6, 190) == 8 and R.code_width(6, 191) == 9
    w, h, m, pay = by["kwkwk_second_code"]
    assert R.read_code(pay, R.code_pos(m, 0) + 3, 3) == 3 and R.read_code(pay, 3 + R.code_pos(m, 1), 3) == 6      # clear, 3, the next free entry
    st = R.stages(by["data_after_full_frame"][3], 3, 13 * 7)
    assert st["status"] == 0 and len(st["pieces"]) == 4 and st["errors"][2] == R.ERR_CODE and st["offsets"][2] == 13 * 7
    assert R.scan(by["no_end_code"][3], 3)[0][-1][2] == R.END_INPUT
    st = R.stages(by["string_across_the_frame_end"][3], 2, 23 * 9)
    assert st["status"] == 0 and sum(st["lengths"]) == 23 * 9 and st["pieces"][-1][2] == R.END_INPUT


def test_damage_list_and_pillow():
    seen = 0
    for name, f in R.damaged():
        d = R.decode(f)
        assert R.plan(f)["supported"] and d["status"] != 0 and d["rgb"] is None, name
        seen |= d["status"]
        with pytest.raises(Exception):                                             # every damaged file makes Pillow raise
            host_decode(f)
        with pytest.raises(R.Damaged):
            R.serial_indices(d["plan"]["payload"], d["plan"]["min_code"], 13 * 7 if "long" not in name else 160 * 120)
    assert seen == R.ERR_FIRST | R.ERR_CODE | R.ERR_SHORT
    # the piece table's room: a stream that clears before every code, longer than the table holds -- stricter than Pillow, which reads it
    m, n = 2, 4200
    pay = R.pack_codes([c for b in R.noisy(n, 1, m, seed=1) for c in (4, b)] + [5], m)
    assert R.piece_cap(len(pay), m) == 4096 and R.scan(pay, m) [1] == R.ERR_PIECES
    f = R.gif_file(70, 60, m, pay, gct=R.colours(4, 1))
    assert R.decode(f)["status"] == R.ERR_PIECES and host_decode(f)[0].shape == (60, 70, 3)


def test_stricter_than_pillow_classes_are_the_named_ones():
    """a refused file keeps the host path whatever Pillow makes of it; the ones Pillow accepts are the named classes"""
    accepted = set()
    for name, f, reason in R.refusals():
        try:
            host_decode(f)
            accepted.add(name)
        except Exception:
            pass
    assert accepted == {"no_terminator", "unknown_block", "code_size_0"}


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_equals_the_walk_field_by_field(good):
    for name, f in [(n, f) for n, f, _ in good] + R.damaged():
        want = R.plan(f)
        got, table = lib_plan(f)
        assert want["supported"] == 1 and got == {k: want[k] for k in R.PLAN_FIELDS} and table == want["table"], name
    by = {n: d["plan"] for n, _, d in good}
    assert by["local_over_global"]["local_table"] == 1 and by["ramp_global"]["mode_l"] == 1 and by["no_table"]["table_len"] == 0
    assert by["transparency_no_flag"]["transparency"] == -1 and by["extensions"]["transparency"] == 3 and by["frame_past_t5_i1"]["transparency"] == 5


def test_plan_refuses_reason_by_reason():
    seen = set()
    for name, f, reason in R.refusals():
        want = R.plan(f)
        assert want["reason"] == reason and not want["supported"], (name, R.REASONS[want["reason"]])
        assert lib_plan(f)[0] == {k: want[k] for k in R.PLAN_FIELDS}, name
        seen.add(reason)
    assert seen == set(range(1, len(R.REASONS)))                                   # every reason of bbocr.h on a file of its own


def test_refused_files_keep_the_host_path():
    from bb_ocr_amd.reader import gif_page

    assert all(gif_page(f) is None for _, f, _ in R.refusals())
    assert gif_page(dict(R.handbuilt())["frame_past_tNone_i0"]).shape == (7, 9, 3)
    assert gif_page(b"") is None and gif_page("/no/such/file.gif") is None


def test_reason_constants_and_piece_room_match_the_library():
    import os
    import re

    from bb_ocr_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "bbocr.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"BBOCR_GIF_(\w+) = (\d+)", text)}
    assert header == {n: i for i, n in enumerate(R.REASONS)} == {n: getattr(_lib, "GIF_" + n) for n in R.REASONS}
    lib = _lib.load()
    for nbytes in (0, 1, 100, 65535, 65536, 70000, 10 ** 7):
        for m in range(2, 9):
            assert lib.bbocr_gif_piece_room(nbytes, m) == R.piece_cap(nbytes, m)
    assert lib.bbocr_gif_piece_room(100, 9) == 0


def test_abi_exports():
    from bb_ocr_amd import _lib

    lib = _lib.load()
    for name in ("bbocr_host_gif_plan", "bbocr_gif_decode", "bbocr_op_gif_decode_stage"):
        assert getattr(lib, name) is not None
    plan = _lib.bbocr_gif_plan()
    assert lib.bbocr_host_gif_plan(None, 0, C.byref(plan)) == -1 and lib.bbocr_host_gif_plan(b"GIF8", 4, None) == -1      # BBOCR_ERR_ARG


def test_option_is_off_by_default(monkeypatch):
    from bb_ocr_amd import reader as M

    monkeypatch.delenv("BBOCR_GIF_DECODE", raising=False)
    assert M.gif_decode_enabled() is False and M.gif_decode_enabled(True) is True
    monkeypatch.setenv("BBOCR_GIF_DECODE", "1")
    assert M.gif_decode_enabled() is True and M.gif_decode_enabled(False) is False
