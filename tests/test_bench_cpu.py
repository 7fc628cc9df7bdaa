"""CPU: the pieces of bench.py that decide what the JSON line says (no GPU work): the parity counter behind `parity_in_run`, the
config table, the seeded page set."""
import numpy as np


def test_parity_counter_counts_boxes_texts_and_pages():
    import bench

    box = lambda x: [[x, 0], [x + 9, 0], [x + 9, 5], [x, 5]]
    want = [[(box(0), "alpha", 0.9), (box(20), "beta", 0.8)], [(box(5), "gamma", 0.7)], []]
    same = [[(box(0), "alpha", 0.91), (box(20), "beta", 0.5)], [(box(5), "gamma", 0.7)], []]
    p = bench.parity(want, same, "mixed")
    assert p["all_identical"] and p["boxes_identical"] == "3/3" and p["texts_identical"] == "3/3" and p["pages_identical"] == "3/3"
    assert p["first_text_difference"] is None and p["mode"] == "mixed"          # confidences do not enter: boxes and strings do
    off = [[(box(0), "alpha", 0.9), (box(21), "beta", 0.8)], [(box(5), "gamna", 0.7)], []]
    p = bench.parity(want, off, "bf16")
    assert not p["all_identical"] and p["boxes_identical"] == "2/3" and p["texts_identical"] == "2/3" and p["pages_identical"] == "1/3"
    assert p["first_text_difference"] == {"oracle": "gamma", "gpu": "gamna"}
    # a page with a missing box can never count as identical, free (float) boxes compare as numbers
    fl = [[([[0.5, 0.0], [9.5, 0.0], [9.5, 5.0], [0.5, 5.0]], "x", 0.5)]]
    assert bench.parity(fl, [[([[0.5, 0], [9.5, 0], [9.5, 5], [0.5, 5]], "x", 0.4)]], "fp16")["all_identical"]
    assert bench.parity(want[:1], [[(box(0), "alpha", 0.9)]], "fp16")["pages_identical"] == "0/1"


def test_configs_name_the_baseline_workloads():
    import bench

    assert bench.CONFIGS["p1"][:3] == (1280, 960, 64) and "configs[2]" in bench.CONFIGS["p1"][6]
    assert bench.CONFIGS["a4"][:3] == (2480, 3504, 16) and bench.CONFIGS["a4"][5] == "fp16" and "configs[4]" in bench.CONFIGS["a4"][6]
    assert set(bench.DTYPE) == {"bf16", "fp16", "exact", "mixed", "exact_rec"} and bench.PEAK_BF16_TFLOPS == 2500.0
    assert abs(bench.CRAFT_GFLOP_PER_PAGE["p1"] - 874.22) < 1e-9 and abs(bench.CRAFT_GFLOP_PER_PAGE["a4"] - 3322.03) < 1e-9


def test_rendered_pages_are_seeded_and_distinct():
    import bench

    a = bench.render_pages("p1", 320, 192, 3, 0, 3, 3)
    b = bench.render_pages("p1", 320, 192, 3, 0, 3, 3)
    assert len(a) == 3 and all(np.array_equal(x, y) for x, y in zip(a, b))          # same seeds -> same pages (every rank, every run)
    assert not np.array_equal(a[0], a[1]) and a[0].shape == (192, 320, 3) and a[0].dtype == np.uint8
    assert np.array_equal(a[0][..., 0], a[0][..., 1]) and not np.array_equal(a[1][..., 0], a[1][..., 1])      # every other page on tinted stock
    assert np.array_equal(bench.render_pages("p1", 320, 192, 3, 1, 2, 2)[0], a[1])                              # a shard starts at its global index


def test_plain_run_does_only_the_headline_and_full_restores_the_extras():
    import bench

    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.legs, a.cpu_pages, a.dump_outputs) == (7, 3, False, "", 0, None)
    f = bench.parse_args(["--steps", "7", "--full"])
    assert f.full and f.legs == bench.FULL_LEGS and f.cpu_pages == bench.FULL_CPU_PAGES == 16
    assert set(f.legs.split(",")) == {"serial", "mixed", "exact", "exact_rec", "a4", "det_only", "single_page", "host_pages", "lowconf", "preprocess", "extractor"}
    e = bench.parse_args(["--legs", "serial", "--cpu-pages", "2", "--dump-outputs", "out"])        # single extras stay selectable without --full
    assert (e.full, e.legs, e.cpu_pages, e.dump_outputs) == (False, "serial", 2, "out")
    assert bench.parse_args(["--full", "--legs", "", "--cpu-pages", "0"]).legs == ""


def test_dump_outputs_writes_the_result_as_float_arrays(tmp_path):
    import bench

    box = lambda x: [[x, 0], [x + 9, 0], [x + 9, 5], [x, 5]]
    free = [[0.5, 1.25], [9.5, 0.0], [9.5, 5.0], [0.5, 6.0]]
    pages = [[(box(0), "alpha", 0.9), (free, "€5", 0.25)], [], [(box(7), "b", 0.5)]]
    assert bench.dump_outputs(str(tmp_path / "d"), pages) == 3
    got = {n: np.load(tmp_path / "d" / f"{n}.npy") for n in ("boxes", "confidences", "boxes_per_page", "text_codepoints")}
    assert got["boxes"].dtype == got["confidences"].dtype == got["boxes_per_page"].dtype == np.float64 and got["text_codepoints"].dtype == np.float32
    assert np.array_equal(got["boxes"], np.array([box(0), free, box(7)], dtype=np.float64)) and got["boxes"].shape == (3, 4, 2)
    assert np.array_equal(got["confidences"], [0.9, 0.25, 0.5]) and np.array_equal(got["boxes_per_page"], [2, 0, 1])
    assert got["text_codepoints"].shape == (3, 5)
    assert ["".join(chr(int(c)) for c in row if c) for row in got["text_codepoints"]] == ["alpha", "€5", "b"]
    # over the size limit: a fixed prefix of the pages (halved until it fits), never a partial page
    many = [[(box(i), "x" * 40, 0.5)] * 10 for i in range(8)]
    assert bench.dump_outputs(str(tmp_path / "s"), many, limit=5000) == 2          # 232 B per box, 2,328 B per page
    assert np.array_equal(np.load(tmp_path / "s" / "boxes_per_page.npy"), [10, 10])
    assert bench.dump_outputs(str(tmp_path / "e"), [[], []]) == 2 and np.load(tmp_path / "e" / "boxes.npy").shape == (0, 4, 2)
