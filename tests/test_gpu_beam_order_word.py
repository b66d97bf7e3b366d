"""The beam word: k_shade(b - 1) stores, by queue position, the beam code (dominant axis, sign: beam_dir in csrc/mcrt_device.h) and the medium of the ray it
queues, and k_beam_rank(b) sorts by that word, the queue word and from_tri instead of rebuilding the ray from its state; k_beam_scan lays the segments out in
one workgroup per 256 counters.  The method is tests/test_gpu_beam_order.py's (its helpers are used as they are): bounces 2-4 forced by beams and ordered
(MCRT_BEAM_B1=2 MCRT_BEAM_LAST=4 MCRT_BEAM_ORDER=0x1c) against the beams off (MCRT_BEAM_B1=0) -- the hit table and counts of a debug call and the RF images
of a pass of F frames as int32, EQUAL; liver(3), E = 8, S = 256, F = 3, MCRT_PATH_MAX=0 unless the case says otherwise.

Every case runs with MCRT_BEAM_PAIRS=1.  Per ordered bounce: mcrt_debug_beam_order says the bounce WAS ordered (no case passes with nothing ordered), rays
placed = the bounce's ray count, and the (wavefront, beam) pairs k_beam_test's first pass met <= (placed + pads) / 64: one beam per wavefront.  k_beam_test
finds a ray's beam from its state, so a word whose code differed from beam_ray's would put two of ITS beams into one wavefront of the order -- with the
spacing (1.0, 0.5, 2.0), where the dominant axis of the segment is not that of the direction, this pins k_shade's code to k_beam_test's."""
import pytest

import test_gpu_beam_order as bo
from test_gpu_constants import _moved

pytestmark = pytest.mark.gpu

ORDERED = (2, 3, 4)


def env(**more):
    return bo.forced(4, bo.DEEP, MCRT_BEAM_PAIRS=1, **more)


CASES = {
    # 256 slots x 6 + 1 = 1537 counters: seven workgroups of k_beam_scan, the last holds the pseudo-beam alone
    "table_256": bo.Case("liver", env(MCRT_BEAM_GROUPS=256), (1, 2, 3, 4)),
    # 3073 counters: thirteen workgroups
    "table_512": bo.Case("liver", env(MCRT_BEAM_GROUPS=512), (1, 2, 3, 4)),
    # 7 counters; nearly every ray in the pseudo-beam
    "one_group": bo.Case("liver", env(MCRT_BEAM_GROUPS=1), (1, 2, 3, 4), expect="one_group"),
    # ragged segments
    "s96": bo.Case("liver", env(MCRT_BEAM_GROUPS=256), (1, 2, 3, 4), S=96, pads=True),
    # a scan-line shard: the key's scan-line is relative to the shard
    "shard": bo.Case("liver", env(), (1, 2, 3, 4), E=12, e0=4, e1=12),
    # a bounce without rays: an order of length 0
    "sphere": bo.Case("sphere", env(), (1, 2, 3, 4)),
    # the components of the segment scaled differently: the code comes from the segment, not from the direction
    "spacing": bo.Case("liver_spaced", env(), (1, 2, 3, 4), expect="none"),
}


def _spaced(mcrt):
    if "liver_spaced" not in bo._scenes:
        cfg, sd = bo._scene(mcrt, "liver")
        bo._scenes["liver_spaced"] = (cfg, _moved(mcrt, sd, spacing=(1.0, 0.5, 2.0)))


@pytest.mark.parametrize("name", list(CASES))
def test_ordered_by_the_stored_word_bit_identical(mcrt, name):
    case = CASES[name]
    _spaced(mcrt)
    off, on = bo._beams_off(mcrt, case), bo._run(mcrt, case, case.env)
    assert case.ordered == ORDERED
    for which in (4, 5):      # the debug call, the pass
        for b in ORDERED:
            (ran, decided, walked, *_), (ordered, placed, segments, pads, met) = on[which][b]
            print("%s %s bounce %d: %d decided %d walked | ordered %s placed %d segments %d pads %d pairs %d" % (name, ("debug call", "pass")[which - 4], b, decided, walked, ordered, placed, segments, pads, met))
            assert ran and ordered, (name, which, b)
            assert placed == decided + walked, (name, which, b, placed, decided, walked)
            assert met <= (placed + pads) // 64, (name, which, b, met, placed, pads)
    bo._check(case, name, off, on, pairs=True)
    if name == "spacing":      # the beams carry the case: most rays of bounce 2 of the pass are decided by lists, in more than one beam
        (_, decided, walked, _, _, used, _, _), (_, placed, segments, _, met) = on[5][2]
        assert decided > 0 and segments > 1 and met > 0, (decided, walked, used, segments, met)
