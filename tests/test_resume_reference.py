"""Conditions on the inputs of the modulation tests of tests/test_gpu_resume.py that need no device, as
tests/test_temper_reference.py keeps them for its runs: on the chosen weights, seed frames, labels and Philox seed, the
float32 frame loop with the label switch parts from the float64 one in at most FLIP_CAP notes, all of them within the
near-flip window; and the switch is visible, so the GPU test's "frames after the boundary differ" can hold."""
import numpy as np
import pytest

import resume_reference as RR
import temper_reference as TR


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_float32_modulated_run_stays_within_the_flip_cap(which):
    fol, got = RR.flips_f32_against_f64(which)
    print("%s: %d flips, %d outside the window of %.1e" % (which, fol.flips, fol.far, fol.win))
    assert fol.far == 0 and fol.clamp_wrong == 0
    assert fol.flips <= TR.FLIP_CAP
    assert got.shape[1] == sum(RR.PLAN_FRAMES) and set(np.unique(got)) <= {0.0, 1.0} and 0 < got.mean() < 1


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_the_label_switch_changes_the_piece(which):
    p, seeds, w, L, gen = RR.case(which)
    plan = RR.plan_of(w)
    assert not np.array_equal(plan[0][0], plan[1][0]) and np.all(plan[1][0].sum(1) == 1)
    assert np.all(plan[0][0].argmax(1) != plan[1][0].argmax(1))            # every piece changes its key
    n0, n1 = RR.PLAN_FRAMES
    mod = gen(p, seeds, plan, RR.MOD_SEED[which], L)
    same = gen(p, seeds, [(plan[0][0], n0 + n1)], RR.MOD_SEED[which], L)
    assert np.array_equal(mod[:, :n0], same[:, :n0]) and not np.array_equal(mod[:, n0:], same[:, n0:])
    # and the loop without a switch is temper_reference's own
    ref = (TR.vrnn_generate if which == 'cl_vrnn' else TR.vae_generate)(p, seeds, w, n0 + n1, RR.MOD_SEED[which], L)[0]
    assert np.array_equal(same, ref)
