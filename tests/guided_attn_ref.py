"""Float64 NumPy reference of the guided attention loss and the alignment scores (include/nspeech_hip.h,
ns_guided_attention).  For utterance n with T_n encoder positions and S_n decoder steps:

    W_n[s,t] = 1 - exp(-(t/T_n - s/S_n)^2 / (2 sigma^2))          0 <= s < S_n, 0 <= t < T_n
    G_n      = 1/(S_n T_n) sum_{s,t} align[n,s,t] W_n[s,t]
    F_n      = 1/S_n sum_s max_{t<T_n} align[n,s,t]
    L_att    = mean_n G_n,   focus = mean_n F_n
    d(weight L_att)/d align[n,s,t] = weight W_n[s,t] / (N S_n T_n)   on the valid region, zero elsewhere

`align` is [N, S, T] here (step s of utterance n in row s); the kernels' slot layout is the caller's business."""
import numpy as np


def out_steps(target_lengths, outputs_per_step, S):
    """S_n = min(S, max(1, ceil(frames_n / r))); None -> S for every row."""
    tl = np.asarray(target_lengths, np.int64)
    return np.minimum(S, np.maximum(1, -(-tl // int(outputs_per_step)))).astype(np.int64)


def weights(T_n, S_n, sigma):
    """W_n as float64 [S_n, T_n]."""
    t = np.arange(T_n, dtype=np.float64)[None, :] / float(T_n)
    s = np.arange(S_n, dtype=np.float64)[:, None] / float(S_n)
    return 1.0 - np.exp(-(t - s) ** 2 / (2.0 * float(sigma) ** 2))


def torch_loss(alignments, in_lengths, steps, sigma):
    """L_att of a float64 oracle's `alignments` [N, T_in, steps] as a differentiable torch scalar (the oracle tests add
    weight * this to the oracle's loss before backward()); steps None: every row spans all steps."""
    import torch
    N, _, S = alignments.shape
    tot = 0.0
    for n in range(N):
        T_n, S_n = int(in_lengths[n]), S if steps is None else int(steps[n])
        W = torch.tensor(weights(T_n, S_n, sigma), dtype=alignments.dtype)                     # [S_n, T_n]
        tot = tot + (alignments[n, :T_n, :S_n] * W.t()).sum() / float(S_n * T_n)
    return tot / N


def torch_focus(alignments, in_lengths, steps):
    import torch
    N, _, S = alignments.shape
    f = [alignments[n, :int(in_lengths[n]), :(S if steps is None else int(steps[n]))].max(dim=0).values.mean() for n in range(N)]
    return torch.stack(f).mean()


def guided_attention(align, in_lengths, steps=None, sigma=0.4, weight=1.0):
    """align [N, S, T] -> dict(W=[W_n ...], G=[N], F=[N], loss=L_att, focus=..., dalign=[N, S, T] the increment
    weight * dL_att/dalign, zero outside the valid region)."""
    a = np.asarray(align, np.float64)
    N, S, T = a.shape
    Tn = np.asarray(in_lengths, np.int64)
    Sn = np.full(N, S, np.int64) if steps is None else np.asarray(steps, np.int64)
    assert Tn.shape == (N,) and Sn.shape == (N,) and (Tn >= 1).all() and (Tn <= T).all() and (Sn >= 1).all() and (Sn <= S).all()
    Ws, G, F = [], np.zeros(N), np.zeros(N)
    d = np.zeros_like(a)
    for n in range(N):
        W = weights(Tn[n], Sn[n], sigma)
        v = a[n, :Sn[n], :Tn[n]]
        Ws.append(W)
        G[n] = (v * W).sum() / (Sn[n] * Tn[n])
        F[n] = v.max(axis=1).sum() / Sn[n]
        d[n, :Sn[n], :Tn[n]] = float(weight) * W / (N * Sn[n] * Tn[n])
    return dict(W=Ws, G=G, F=F, loss=float(G.mean()), focus=float(F.mean()), dalign=d)
