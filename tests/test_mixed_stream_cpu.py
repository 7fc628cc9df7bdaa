"""CPU: the streaming loop behind Reader.readtext_stream and Reader.readtext_pages_stream (no device: the device call is a stand-in).
Both forms hold a lazy producer to the same back-pressure -- `in_flight` calls running and one batch queued behind them -- so that the
pages of a long call never sit on the card all at once, and both yield each result as soon as it is the next one."""
import pytest


def _reader(calls):
    from bb_ocr_amd.reader import Reader

    r = Reader.__new__(Reader)                       # no context: only the two stand-ins below are called
    r.readtext_device = lambda rgb, gray=None, **kw: calls.append(("device", rgb, gray, kw)) or [("d", rgb, gray)]
    r.readtext_pages = lambda pages, **kw: calls.append(("pages", pages, kw)) or [("p", pg) for pg in pages]
    return r


@pytest.mark.parametrize("form", ["stream", "pages_stream"])
@pytest.mark.parametrize("in_flight", [1, 2, 3])
def test_the_producer_is_drained_one_batch_ahead(form, in_flight):
    calls, made = [], []
    r = _reader(calls)
    n = 9

    def feed():
        for k in range(n):
            made.append(k)
            yield [k, -k] if form == "pages_stream" else (k, -k)

    stream = (r.readtext_pages_stream if form == "pages_stream" else r.readtext_stream)(feed(), in_flight=in_flight, detail=1)
    assert made == []                                # lazy until asked
    got = []
    for k, res in enumerate(stream):
        got.append(res)
        # result k is out: at most in_flight running + one queued behind them have been produced beyond it -- never the whole list
        assert len(made) <= k + 1 + in_flight, (k, made)
    assert made == list(range(n)) and len(got) == n
    if form == "pages_stream":
        assert got == [[("p", k), ("p", -k)] for k in range(n)]
        assert sorted(c[1][0] for c in calls) == list(range(n)) and all(c[0] == "pages" and c[2] == {"detail": 1} for c in calls)
    else:
        assert got == [[("d", k, -k)] for k in range(n)]
        assert all(c[0] == "device" and c[3] == {"detail": 1} for c in calls)


def test_a_failing_call_raises_at_its_place():
    calls = []
    r = _reader(calls)

    def bad(pages, **kw):
        if pages == [2]:
            raise RuntimeError("page list 2")
        return pages

    r.readtext_pages = bad
    stream = r.readtext_pages_stream(iter([[0], [1], [2], [3]]))
    assert next(stream) == [0] and next(stream) == [1]
    with pytest.raises(RuntimeError, match="page list 2"):
        next(stream)
