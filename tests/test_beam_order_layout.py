"""The layout of a beam order (csrc/mcrt_beam.hip: k_beam_scan) as the host evaluates it (mcrt_debug_beam_layout, which shares beam_segment() with the kernel):
an exclusive prefix over the beams' ray counts rounded up to multiples of 64 -- no wavefront of the order straddles two beams --, the pad lanes and the totals,
against numpy on random counts and at the edges: no beams at all, one ray, a count of exactly 64, either side of it, empty beams between full ones."""
import numpy as np
import pytest


def _expect(counts):
    c = np.asarray(counts, np.int64)
    seg = (c + 63) // 64 * 64
    bases = np.concatenate([[0], np.cumsum(seg)[:-1]]) if len(c) else np.zeros(0, np.int64)
    return bases, int(c.sum()), int((c > 0).sum()), int(seg.sum() - c.sum()), int(seg.sum())


EDGES = {
    "no_beams": [],
    "pseudo_beam_alone_empty": [0],
    "one_ray": [1],
    "exactly_64": [64],
    "63_64_65": [63, 64, 65],
    "empty_between": [0, 0, 5, 0, 128, 0, 0, 1, 0],
    "one_ray_in_the_pseudo_beam": [0] * 24576 + [1],
}


@pytest.mark.parametrize("name", list(EDGES))
def test_layout_edges(mcrt, name):
    counts = EDGES[name]
    bases, placed, segments, pads, total = mcrt.host_beam_layout(counts)
    eb, ep, es, epad, et = _expect(counts)
    assert np.array_equal(bases.astype(np.int64), eb) and (placed, segments, pads, total) == (ep, es, epad, et)
    assert total % 64 == 0 and pads <= 63 * segments


@pytest.mark.parametrize("seed", range(4))
def test_layout_random_counts(mcrt, seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 30000))
    counts = rng.integers(0, 5000, n) * (rng.random(n) < 0.2)           # most beams empty, as in the group table
    counts[rng.integers(0, n, 8)] = 64 * rng.integers(1, 9, 8)          # ... and some whole wavefronts
    bases, placed, segments, pads, total = mcrt.host_beam_layout(counts)
    eb, ep, es, epad, et = _expect(counts)
    assert np.array_equal(bases.astype(np.int64), eb) and (placed, segments, pads, total) == (ep, es, epad, et)
    # every segment starts a wavefront, and the segments of the beams that have rays neither overlap nor leave a gap
    assert (bases % 64 == 0).all()
    live = np.flatnonzero(counts)
    assert np.array_equal(bases[live][1:].astype(np.int64), (bases[live] + (np.asarray(counts)[live] + 63) // 64 * 64)[:-1])


def test_layout_refuses_an_order_past_32_bits(mcrt):
    with pytest.raises(Exception):
        mcrt.host_beam_layout([0xffffffc0, 0xffffffc0])
