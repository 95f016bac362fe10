"""tests/guided_attn_ref.py (the float64 contract of ns_guided_attention) against torch float64 autograd and the
properties the definition promises."""
import numpy as np
import torch

import guided_attn_ref as R


def _align(rng, N, S, T):
    a = rng.uniform(0.05, 1.0, size=(N, S, T))
    return a / a.sum(axis=2, keepdims=True)


def _torch_loss(a, Tn, Sn, sigma):
    """L_att written out in torch, independently of the NumPy code: explicit grids per utterance."""
    N = a.shape[0]
    tot = 0.0
    for n in range(N):
        t = torch.arange(int(Tn[n]), dtype=torch.float64)[None, :] / float(Tn[n])
        s = torch.arange(int(Sn[n]), dtype=torch.float64)[:, None] / float(Sn[n])
        W = 1.0 - torch.exp(-(t - s) ** 2 / (2.0 * sigma * sigma))
        tot = tot + (a[n, :int(Sn[n]), :int(Tn[n])] * W).sum() / float(int(Sn[n]) * int(Tn[n]))
    return tot / N


def test_increment_equals_autograd_of_the_weighted_loss():
    rng = np.random.RandomState(0)
    N, S, T = 4, 9, 14
    Tn, Sn = np.array([14, 9, 3, 1]), np.array([9, 4, 1, 6])
    for sigma, weight in ((0.4, 1.0), (0.2, 3.5)):
        a = torch.tensor(_align(rng, N, S, T), dtype=torch.float64, requires_grad=True)
        loss = weight * _torch_loss(a, Tn, Sn, sigma)
        loss.backward()
        ref = R.guided_attention(a.detach().numpy(), Tn, Sn, sigma=sigma, weight=weight)
        assert np.abs(ref["dalign"] - a.grad.numpy()).max() <= 1e-12
        assert abs(weight * ref["loss"] - float(loss.detach())) <= 1e-12
        # nothing outside the valid region
        for n in range(N):
            assert not ref["dalign"][n, Sn[n]:].any() and not ref["dalign"][n, :, Tn[n]:].any()


def test_weight_is_zero_on_the_diagonal_and_positive_off_it():
    for T_n, S_n in ((8, 8), (12, 4), (5, 15), (160, 200)):
        W = R.weights(T_n, S_n, 0.4)
        assert W.shape == (S_n, T_n)
        for s in range(S_n):
            for t in range(T_n):
                if t * S_n == s * T_n:          # t/T_n = s/S_n
                    assert W[s, t] == 0.0
                else:
                    assert 0.0 < W[s, t] < 1.0


def test_row_losses_lie_in_the_unit_interval():
    rng = np.random.RandomState(1)
    N, S, T = 5, 11, 17
    Tn, Sn = rng.randint(1, T + 1, N), rng.randint(1, S + 1, N)
    for sigma in (0.05, 0.2, 0.4, 2.0):
        ref = R.guided_attention(_align(rng, N, S, T), Tn, Sn, sigma=sigma)
        assert (ref["G"] >= 0.0).all() and (ref["G"] < 1.0).all()
        assert 0.0 <= ref["loss"] < 1.0
        assert (ref["F"] > 0.0).all() and (ref["F"] <= 1.0).all()
    # the worst alignment there is - all mass in the corner farthest from the diagonal - still stays below 1
    a = np.zeros((1, S, T))
    a[0, :, T - 1] = 1.0
    a[0, S - 1, :] = 0.0
    a[0, S - 1, 0] = 1.0
    assert R.guided_attention(a, [T], [S], sigma=0.01)["G"][0] < 1.0


def test_focus_is_one_for_one_hot_rows_and_the_diagonal_costs_nothing():
    N, S, T = 2, 6, 6
    a = np.zeros((N, S, T))
    for s in range(S):
        a[0, s, s] = 1.0                    # the diagonal
        a[1, s, (3 * s + 1) % T] = 1.0      # one-hot, but scattered
    ref = R.guided_attention(a, [T, T], None, sigma=0.4)
    assert ref["F"][0] == 1.0 and ref["F"][1] == 1.0 and ref["focus"] == 1.0
    assert ref["G"][0] == 0.0 and ref["G"][1] > 0.0
    # a uniform row has focus 1 / T_n
    u = np.full((1, S, T), 1.0 / T)
    assert abs(R.guided_attention(u, [T], None)["F"][0] - 1.0 / T) < 1e-15


def test_length_one_edges():
    rng = np.random.RandomState(2)
    a = _align(rng, 2, 5, 7)
    # T_n = 1: the single column sits at t/T_n = 0, W[s, 0] = 1 - exp(-(s/S_n)^2 / (2 sigma^2))
    ref = R.guided_attention(a, [1, 7], [5, 1], sigma=0.3)
    W0 = ref["W"][0]
    assert W0.shape == (5, 1) and W0[0, 0] == 0.0
    assert np.allclose(W0[:, 0], 1.0 - np.exp(-(np.arange(5) / 5.0) ** 2 / (2 * 0.09)), rtol=0, atol=1e-15)
    assert abs(ref["G"][0] - (a[0, :5, 0] * W0[:, 0]).sum() / 5.0) < 1e-15
    assert abs(ref["F"][0] - a[0, :5, 0].mean()) < 1e-15
    # S_n = 1: the single step sits at s/S_n = 0
    W1 = ref["W"][1]
    assert W1.shape == (1, 7) and W1[0, 0] == 0.0
    assert abs(ref["G"][1] - (a[1, 0, :7] * W1[0]).sum() / 7.0) < 1e-15
    assert abs(ref["F"][1] - a[1, 0, :7].max()) < 1e-15
    assert not ref["dalign"][0, :, 1:].any() and not ref["dalign"][1, 1:].any()


def test_steps_from_frame_counts():
    # r = 5, S = 8: 40 frames -> 8, 33 -> ceil(6.6) = 7 (not a multiple of r), 5 -> 1, 4 -> 1, 0 -> 1 (never 0),
    # 41 and more -> clamped to S
    assert R.out_steps([40, 33, 5, 4, 0, 41, 1000], 5, 8).tolist() == [8, 7, 1, 1, 1, 8, 8]
    assert R.out_steps([20, 12, 3], 5, 4).tolist() == [4, 3, 1]
    assert R.out_steps([7], 1, 50).tolist() == [7]
    # steps=None is S for every row
    rng = np.random.RandomState(3)
    a = _align(rng, 2, 4, 6)
    x, y = R.guided_attention(a, [6, 3], None), R.guided_attention(a, [6, 3], [4, 4])
    assert x["loss"] == y["loss"] and np.array_equal(x["dalign"], y["dalign"])


def test_torch_helpers_agree_with_the_numpy_reference():
    """torch_loss / torch_focus take an oracle's alignments [N, T_in, steps]; the GPU model tests add them to the oracles'
    losses, so they must be the reference's L_att and focus."""
    rng = np.random.RandomState(4)
    N, S, T = 3, 6, 10
    a = _align(rng, N, S, T)
    Tn, Sn = np.array([10, 7, 2]), np.array([6, 2, 5])
    al = torch.tensor(a.transpose(0, 2, 1).copy(), dtype=torch.float64)
    for steps in (Sn, None):
        ref = R.guided_attention(a, Tn, steps, sigma=0.3)
        assert abs(float(R.torch_loss(al, Tn, steps, 0.3)) - ref["loss"]) < 1e-14
        assert abs(float(R.torch_focus(al, Tn, steps)) - ref["focus"]) < 1e-14
