"""CPU: the numpy restatement of the routing (tests/readroute_ref.py) against a segment-by-segment loop, and that its texts hold what the
GPU tests mean them to hold.  No code under test runs here."""
import numpy as np

import readroute_ref as rr


def test_restatement_equals_the_loop_on_every_small_case():
    for name, (text, bounds, bins, check_from, planted) in rr.cases().items():
        outs, bad = rr.route(text, bounds, bins, rr.FIRST, check_from)
        assert sum(map(len, outs)) == len(text), name                      # every byte leaves exactly once
        assert bad == planted, name
        if len(bins) <= 5000:
            assert (outs, bad) == rr.route_loop(text, bounds.tolist(), bins.tolist(), rr.FIRST, check_from), name
        for b in range(3):
            assert len(outs[b]) == int(np.diff(bounds)[bins == b].sum()), name


def test_cases_hold_what_they_are_meant_to_hold():
    c = rr.cases()
    assert sorted(c) == sorted(rr.CASE_NAMES)
    size = lambda name: np.diff(c[name][1])                                # noqa: E731
    assert len(c["one_segment"][2]) == 1 and len(c["one_byte"][0]) == 1
    assert not (c["empty_bin"][2] == 1).any() and (c["empty_bin"][2] == 0).any() and (c["empty_bin"][2] == 2).any()
    assert (size("random") == 0).sum() > 50 and (size("zero_lengths") == 0).sum() == 8
    assert set(size("small_sizes").tolist()) == {1, 15, 16, 17}
    assert size("long_record").max() == 100000 and size("long_record")[20] == 100000
    assert [len(c["text_of_%d" % n][0]) for n in (4095, 4096, 4097)] == [4095, 4096, 4097]
    assert [len(c["scan_pass_%+d" % d][2]) for d in (-1, 0, 1)] == [rr.BLOCK * rr.SCAN_PASS_BLOCKS + d for d in (-1, 0, 1)]
    a, b = c["wrong_first_bytes_from_0"], c["wrong_first_bytes_from_1"]
    assert a[0] == b[0] and a[4] == b[4] + 1 >= 20                         # the first segment's wrong byte counts from 0 only
    # a '@' stands at a segment's first byte and nowhere else
    text, bounds = c["random"][0], c["random"][1]
    at = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == rr.FIRST)
    assert set(at.tolist()) == set(bounds[:-1][np.diff(bounds) > 0].tolist())
