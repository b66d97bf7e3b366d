"""k_beam_scan (csrc/mcrt_beam.hip) run ALONE on given counters (mcrt_debug_beam_scan) against the host's statement of the same layout
(mcrt_debug_beam_layout): a workgroup owns 256 counters, sums the segments before its own by itself and waits for no other; the last one writes the totals.
Compared: every base, rays placed, segments, pad lanes, the order's length -- and the order buffer, which the debug call fills with a sentinel first: the words
[base + count, base + segment) of every beam are the pad word, every other word (the rays' own places, and 64 guard words past the length) still holds the sentinel.

Lengths: one counter, two, either side of one workgroup (255, 256, 257) and of four (1023, 1024, 1025), one counter in the last workgroup (513, 2049),
3073 = 512 groups x 6 + 1 (the pseudo-beam alone in the last workgroup), and the headline table's 24 577."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 255, 256, 257, 513, 1023, 1024, 1025, 2049, 3073, 24577]


def _random(seed):
    def make(n):
        rng = np.random.default_rng(seed)
        return rng.integers(0, 201, n) * (rng.random(n) < 0.5)
    return make


def _only(where):
    def make(n):
        c = np.zeros(n, np.int64); c[where] = 77
        return c
    return make


CONTENTS = {
    "all_0": lambda n: np.zeros(n, np.int64),
    "all_1": lambda n: np.ones(n, np.int64),
    "all_64": lambda n: np.full(n, 64, np.int64),
    "63_64_65": lambda n: np.resize(np.array([63, 64, 65], np.int64), n),
    "first_only": _only(0),
    "last_only": _only(-1),
    "random_0": _random(0), "random_1": _random(1), "random_2": _random(2), "random_3": _random(3),
}


@pytest.fixture(scope="module")
def ctx(mcrt):
    c = mcrt.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("n", LENGTHS)
def test_scan_alone_matches_the_host_layout(mcrt, ctx, n, content):
    counts = np.asarray(CONTENTS[content](n), np.uint32)
    assert len(counts) == n
    hb, hplaced, hsegs, hpads, hlen = mcrt.host_beam_layout(counts)
    bases, placed, segs, pads, length, order = ctx.debug_beam_scan(counts)
    print("n %d %s: device placed %d segments %d pads %d length %d | host %d %d %d %d" % (n, content, placed, segs, pads, length, hplaced, hsegs, hpads, hlen))
    assert np.array_equal(bases, hb), "bases differ at %s" % np.flatnonzero(bases != hb)[:8]
    assert (placed, segs, pads, length) == (hplaced, hsegs, hpads, hlen)
    assert len(order) == hlen + 64
    # the order buffer: pads where the host's layout has them, the sentinel everywhere else
    expect = np.full(hlen + 64, mcrt.api.BEAM_SCAN_SENTINEL, np.uint32)
    c64 = counts.astype(np.int64)
    seg = (c64 + 63) // 64 * 64
    for k in np.flatnonzero(seg != c64):
        expect[int(hb[k]) + int(c64[k]):int(hb[k]) + int(seg[k])] = mcrt.api.BEAM_PAD
    assert int((expect == mcrt.api.BEAM_PAD).sum()) == hpads
    assert np.array_equal(order, expect), "order words differ at %s" % np.flatnonzero(order != expect)[:8]
