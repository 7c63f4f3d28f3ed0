"""tools/p2_trip_model.py: the host model of P2's stencil ranges and wave trip counts."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "repic-copy_amd"))


def test_ranges_hold_every_edge_partner_and_loop_shapes_are_ordered():
    import p2_trip_model as m
    from repic_amd import synth
    cfg = synth.SynthConfig(**synth.CONFIGS["C2"], seed=0)
    B = float(cfg.box)
    for mg in synth.batch(cfg, 3):
        ln, pk, order = m.box_ranges(mg, B)
        xs = np.concatenate([t[0] for t in mg])[order]
        ys = np.concatenate([t[1] for t in mg])[order]
        # a box's ranges hold at least its JI > 0.3 partners among the higher pickers
        for t in range(0, len(xs), 7):
            ox = np.maximum((np.minimum(xs[t], xs) + B) - np.maximum(xs[t], xs), 0)
            oy = np.maximum((np.minimum(ys[t], ys) + B) - np.maximum(ys[t], ys), 0)
            inter = ox * oy
            n_edge = int(((inter / (2 * B * B - inter) > 0.3) & (pk > pk[t])).sum())
            assert ln[t].sum() >= n_edge
        assert (ln[pk == cfg.k - 1] == 0).all()
        rg, pg, fl, pf = m.wave_iterations(ln, 512)
        assert rg >= pg >= fl >= pf > 0


def test_model_reproduces_the_recorded_c2_prediction():
    import p2_trip_model as m
    # wave iterations of 40 micrographs: 130.8 / 96.9 / 94.55 per micrograph
    rg, pg, fl, pf = (int(round(v * 40)) for v in m.model("C2", 512, 40))
    assert (rg, pg, fl) == (5232, 3875, 3782)
