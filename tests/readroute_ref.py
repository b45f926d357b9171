"""The routing of the second pass of `triobin --write-reads` (include/jasper_hip.h: jasper_route_text) restated with numpy, and the texts
the GPU tests route.  A text of n bytes is cut into segments by bounds[n_seg + 1]; segment i has bin code bins[i] in 0..2; each bin's
output is its segments back to back in input order.  A mismatch is a segment i >= check_from that holds a byte and does not begin with
`first`.  tests/test_readroute_ref.py checks this file against a segment-by-segment loop; nothing here is the code under test."""
import numpy as np

BLOCK = 4096                    # text bytes of a workgroup of the copy kernel, and segments of one block of the scans
SCAN_PASS_BLOCKS = 1024         # block totals one pass of the top scan takes
FIRST = ord("@")
CASE_NAMES = ["random", "one_segment", "one_byte", "empty_bin", "all_in_bin_0", "all_in_bin_1", "all_in_bin_2", "zero_lengths", "only_zero_lengths_but_one", "small_sizes",
              "long_record", "text_of_4095", "text_of_4096", "text_of_4097", "segments_4095", "segments_4096", "segments_4097", "scan_pass_-1", "scan_pass_+0", "scan_pass_+1",
              "wrong_first_bytes_from_0", "wrong_first_bytes_from_1"]      # what cases() makes (test_readroute_ref.py holds the two together)


def route(text, bounds, bins, first=FIRST, check_from=0):
    """-> ([bytes, bytes, bytes], mismatches)"""
    buf = np.frombuffer(bytes(text), dtype=np.uint8)
    bounds, bins = np.asarray(bounds, dtype=np.int64), np.asarray(bins, dtype=np.uint8)
    assert len(bounds) == len(bins) + 1 and bounds[0] == 0 and bounds[-1] == len(buf) and (np.diff(bounds) >= 0).all() and (bins < 3).all()
    size = np.diff(bounds)
    code = np.repeat(bins, size)
    outs = [buf[code == b].tobytes() for b in range(3)]
    has = size > 0
    has[:check_from] = False
    begins = bounds[:-1][has]
    return outs, int((buf[begins] != first).sum())


def route_loop(text, bounds, bins, first=FIRST, check_from=0):
    """the same, one segment at a time"""
    outs, bad = [bytearray(), bytearray(), bytearray()], 0
    for i, b in enumerate(bins):
        seg = text[bounds[i]:bounds[i + 1]]
        outs[b] += seg
        if i >= check_from and len(seg) and seg[0] != first:
            bad += 1
    return [bytes(o) for o in outs], bad


def build(sizes, bins, seed, wrong=()):
    """a text for the segment sizes: letters and line feeds, every segment that holds a byte begins with '@' -- but those listed in
    `wrong`, which begin with '#'; no other byte is '@' -> (text, bounds, bins)"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    bounds = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=bounds[1:])
    buf = np.frombuffer(b"ACGTNacgt\n\r+I!", dtype=np.uint8)[rng.integers(0, 14, int(bounds[-1]))]
    has = sizes > 0
    buf[bounds[:-1][has]] = FIRST
    for i in wrong:
        assert sizes[i] > 0
        buf[bounds[i]] = ord("#")
    return buf.tobytes(), bounds, np.asarray(bins, dtype=np.uint8)


def cases():
    """name -> (text, bounds, bins, check_from, planted mismatches the check must count)"""
    rng = np.random.default_rng(11)
    out = {}

    def add(name, sizes, bins, seed, wrong=(), check_from=0):
        text, bounds, bins = build(sizes, bins, seed, wrong)
        out[name] = (text, bounds, bins, check_from, sum(1 for i in wrong if i >= check_from))

    n = 3000
    sizes = rng.integers(0, 600, n)
    sizes[sizes < 40] = 0                               # some empty ones among them
    add("random", sizes, rng.integers(0, 3, n), 1)
    add("one_segment", [70000], [1], 2)
    add("one_byte", [1], [2], 3)
    add("empty_bin", rng.integers(1, 500, 800), rng.integers(0, 2, 800) * 2, 4)      # no segment of bin 1
    for b in range(3):
        add("all_in_bin_%d" % b, rng.integers(1, 500, 800), np.full(800, b), 5 + b)
    add("zero_lengths", [0, 0, 5, 0, 0, 0, 31, 0, 16, 0, 0], [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1], 8)
    add("only_zero_lengths_but_one", [0] * 40 + [33] + [0] * 40, [i % 3 for i in range(81)], 9)
    add("small_sizes", [1, 15, 16, 17] * 300 + [17, 16, 15, 1] * 300, rng.integers(0, 3, 2400), 10)
    add("long_record", [300] * 20 + [100000] + [300] * 20, [i % 3 for i in range(41)], 11)
    for n in (BLOCK - 1, BLOCK, BLOCK + 1):
        add("text_of_%d" % n, [n - 1000, 1000], [0, 2], 12)
        add("segments_%d" % n, rng.integers(0, 3, n), rng.integers(0, 3, n), 13)
    for d in (-1, 0, 1):                                # one segment less than a pass of the top scan takes, as many, one more
        n = BLOCK * SCAN_PASS_BLOCKS + d
        add("scan_pass_%+d" % d, np.arange(n) % 3, (np.arange(n) // 7) % 3, 14)
    sizes = rng.integers(1, 400, 2000)
    wrong = sorted(set(rng.integers(0, 2000, 25).tolist()) | {0, 1999})
    add("wrong_first_bytes_from_0", sizes, rng.integers(0, 3, 2000), 15, wrong, 0)
    add("wrong_first_bytes_from_1", sizes, rng.integers(0, 3, 2000), 15, wrong, 1)
    return out
