"""tests/stop_token_ref.py (the float64 contract of ns_stop_token) against torch float64 autograd and hand-made cases."""
import numpy as np
import torch

import stop_token_ref as R

FRAMES = (20, 12, 3)            # frames before padding, outputs_per_step 5, S = 4 -> S_n = (4, 3, 1)


def test_targets_of_the_model_tests_frames():
    steps = R.out_steps(FRAMES, 5, 4)
    assert steps.tolist() == [4, 3, 1]
    assert R.targets(steps, 4).tolist() == [[0, 0, 0, 1], [0, 0, 1, 1], [1, 1, 1, 1]]
    # steps outside [1, S] are clamped, as the kernel clamps out_steps
    assert R.targets([0, 9], 4).tolist() == [[1, 1, 1, 1], [0, 0, 0, 1]]


def _case(seed, N=3, S=4, D=64):
    rng = np.random.RandomState(seed)
    return rng.standard_normal((N, S, D)), rng.standard_normal(D) * 0.3, rng.standard_normal(1)


def test_closed_form_gradients_equal_autograd():
    for seed, steps, pw, gs in ((0, [4, 3, 1], 1.0, 1.0), (1, None, 5.0, 0.7), (2, [1, 1, 4], 0.25, 3.0)):
        h, w, b = _case(seed)
        ref = R.stop_token(h, w, b, steps, pos_weight=pw, grad_scale=gs)
        th, tw, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (h, w, b))
        z = th @ tw + tb
        z.retain_grad()
        sp = torch.nn.functional.softplus
        y = torch.tensor(ref["y"])
        loss = (pw * y * sp(-z) + (1 - y) * sp(z)).sum() / z.numel()
        assert abs(float(loss.detach()) - ref["loss"]) < 1e-14
        assert abs(float(R.torch_loss(th, tw, tb, steps, pw).detach()) - ref["loss"]) < 1e-14
        (gs * loss).backward()
        for got, want in ((ref["dz"], z.grad), (ref["dh"], th.grad), (ref["dw"], tw.grad), (ref["db"], tb.grad)):
            want = want.numpy().reshape(np.shape(got))
            assert np.abs(np.asarray(got) - want).max() <= 1e-14 * max(1.0, np.abs(want).max())


def test_finite_and_right_at_large_logits():
    # one row per sign: h = 1 in one column, w = +-80 there
    h = np.zeros((2, 1, 64)); h[:, 0, 0] = 1.0
    for zval in (80.0, -80.0):
        w = np.zeros(64); w[0] = zval
        for steps, pw in (([1, 1], 3.0), (None, 3.0)):          # both rows positive (S = 1: every step is the last)
            ref = R.stop_token(h, w, [0.0], steps, pos_weight=pw)
            assert np.isfinite(ref["l"]).all() and np.isfinite(ref["dz"]).all() and np.isfinite(ref["dw"]).all()
            want_l = pw * (np.exp(-80.0) if zval > 0 else 80.0 + np.exp(-80.0))
            assert np.allclose(ref["l"], want_l, rtol=1e-12, atol=0.0)
            want_dz = -pw * (np.exp(-80.0) if zval > 0 else 1.0) / 2
            assert np.allclose(ref["dz"], want_dz, rtol=1e-12, atol=0.0)
    # negatives: two steps, S_n = 2, step 0 is negative
    h2 = np.zeros((1, 2, 64)); h2[:, :, 0] = 1.0
    for zval in (80.0, -80.0):
        w = np.zeros(64); w[0] = zval
        ref = R.stop_token(h2, w, [0.0], [2])
        assert np.isfinite(ref["l"]).all() and np.isfinite(ref["dz"]).all()
        assert np.isclose(ref["l"][0, 0], 80.0 + np.exp(-80.0) if zval > 0 else np.exp(-80.0), rtol=1e-12, atol=0.0)
        assert np.isclose(ref["dz"][0, 0], (1.0 if zval > 0 else np.exp(-80.0)) / 2, rtol=1e-12, atol=0.0)


def test_stop_steps_on_hand_made_logits():
    t = R.threshold_logit(0.7)
    assert abs(t - np.log(0.7 / 0.3)) < 1e-15 and R.threshold_logit(0.5) == 0.0
    z = np.full((4, 5), t - 1.0)
    z[1, 0] = t + 1e-9          # step 0 over the threshold
    z[2, 3] = t                 # exactly the threshold: does not count
    z[3, 2] = t + 0.5; z[3, 4] = t + 2.0        # the first crossing decides
    assert R.stop_steps(z, t).tolist() == [5, 1, 5, 3]
    # the step error of the training form is measured at probability 0.5
    h = np.zeros((2, 3, 64)); h[0, 1, 0] = 1.0
    w = np.zeros(64); w[0] = 2.0
    ref = R.stop_token(h, w, [-1.0], [3, 2])
    assert ref["z"].tolist() == [[-1.0, 1.0, -1.0], [-1.0, -1.0, -1.0]]
    assert ref["step_error"] == (abs(2 - 3) + abs(3 - 2)) / 2
