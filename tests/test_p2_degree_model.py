"""tools/p2_trip_model.py --degrees: forward degrees per wave-round (the host model of what the
one-pass P2 list write works on), on a micrograph small enough to check by eye."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from p2_trip_model import box_ranges, degree_report, forward_degrees  # noqa: E402

B = 100.0


def _mg(pickers):
    return [(np.array([p[0] for p in pts], float), np.array([p[1] for p in pts], float),
             np.full(len(pts), 0.5)) for pts in pickers]


def test_forward_degrees_by_eye():
    """Three particles 1000 px apart.  Particle A: one box in picker 0, two in picker 1, one in
    picker 2, all within 10 px: A0 -> A1, A1', A2 (3 edges), A1 -> A2, A1' -> A2.  Particle B:
    one box per picker: B0 -> B1, B2 and B1 -> B2.  Particle C: picker 0 only.  A picker-2
    box far from everything.  8 forward edges; one box with more than two."""
    mg = _mg([[(0, 0), (1000, 0), (2000, 0)],
              [(5, 5), (10, 0), (1005, 0)],
              [(0, 8), (1000, 5), (3000, 500)]])
    ln, pk, order = box_ranges(mg, B)
    deg = forward_degrees(mg, B, order)
    # positions are picker-major and, inside a picker, follow x here (one box per grid column)
    assert pk.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert order.tolist() == list(range(9))
    assert deg.tolist() == [3, 2, 0, 1, 1, 1, 0, 0, 0]
    assert degree_report(deg, 64) == dict(boxes=9, edges=8, slow_boxes=1, wave_rounds=1,
                                          slow_wave_rounds=1, write_trips=3)


def test_wave_rounds_are_aligned_blocks_in_both_directions():
    """130 boxes: blocks 0..63, 64..127 and 128..129, whatever the workgroup size (the odd,
    reversed round of a 64- or 128-thread workgroup covers the same aligned blocks).  Largest
    degrees 4, 2 and 1: 7 write trips; only the first block holds a box with more than two."""
    deg = np.zeros(130, np.int64)
    deg[[0, 63]] = [4, 3]
    deg[[64, 100, 127]] = [2, 1, 2]
    deg[129] = 1
    want = dict(boxes=130, edges=13, slow_boxes=2, wave_rounds=3, slow_wave_rounds=1, write_trips=7)
    assert degree_report(deg, 64) == want
    assert degree_report(deg, 128) == want
    # 512 threads: one round, the same three blocks (five waves hold no box)
    assert degree_report(deg, 512) == want
