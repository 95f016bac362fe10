"""Float64 restatement of the Tacotron-2 stop token (include/nspeech_hip.h, ns_stop_token).  With
z[n,s] = h[n,s,:] . w + b, S_n decoder steps of utterance n, y[n,s] = 1 if s >= S_n - 1 else 0 and
sp(x) = max(x, 0) + log1p(exp(-|x|)):

    l[n,s]  = pos_weight * y * sp(-z) + (1 - y) * sp(z)
    L_stop  = 1/(N S) * sum_{n,s} l[n,s]
    dz[n,s] = grad_scale / (N S) * ((1 - y) * sigma(z) - pos_weight * y * (1 - sigma(z)))
    dh[n,s,:] = dz[n,s] * w      dw = sum_{n,s} dz[n,s] * h[n,s,:]      db = sum_{n,s} dz[n,s]
    S^_n    = 1 + min{ s : z[n,s] > threshold_logit }, or S when no step qualifies

NumPy for the kernel's contract test, torch (inside an autograd graph) for the models' oracle tests."""
import numpy as np
import torch


def out_steps(frames, r, S):
    """S_n = min(S, max(1, ceil(frames[n] / r))): Tacotron2._guided_steps."""
    return np.clip(-(-np.asarray(frames, np.int64) // int(r)), 1, int(S)).astype(np.int32)


def targets(steps, S):
    """y [N, S]: the step that emits the last real frame and every later step are positive."""
    steps = np.clip(np.asarray(steps, np.int64), 1, int(S))
    return (np.arange(int(S))[None, :] >= steps[:, None] - 1).astype(np.float64)


def softplus(x):
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def stop_steps(z, threshold_logit):
    """S^_n [N] of logits z [N, S]; a logit equal to the threshold does not count."""
    z = np.asarray(z, np.float64)
    over = z > threshold_logit
    return np.where(over.any(axis=1), over.argmax(axis=1) + 1, z.shape[1]).astype(np.int64)


def threshold_logit(t):
    return float(np.log(np.float64(t) / (1.0 - np.float64(t))))


def stop_token(h, w, b, steps=None, pos_weight=1.0, grad_scale=1.0):
    """h [N, S, D], w [D], b scalar (any float arrays, widened to float64); steps [N] or None (S for every row).
    Returns dict(z, y, l, loss, dz, dh, dw, db, step_error) in float64."""
    h, w = np.asarray(h, np.float64), np.asarray(w, np.float64).reshape(-1)
    b = float(np.asarray(b, np.float64).reshape(-1)[0])
    N, S, _ = h.shape
    Sn = np.full(N, S, np.int64) if steps is None else np.clip(np.asarray(steps, np.int64), 1, S)
    z = h @ w + b
    y = targets(Sn, S)
    l = pos_weight * y * softplus(-z) + (1.0 - y) * softplus(z)
    dz = grad_scale / (N * S) * ((1.0 - y) * sigmoid(z) - pos_weight * y * sigmoid(-z))
    return dict(z=z, y=y, l=l, loss=float(l.sum() / (N * S)), dz=dz, dh=dz[:, :, None] * w[None, None, :],
                dw=np.einsum("ns,nsd->d", dz, h), db=float(dz.sum()),
                step_error=float(np.abs(stop_steps(z, 0.0) - Sn).mean()))


def torch_loss(h, w, b, steps=None, pos_weight=1.0):
    """L_stop of torch tensors h [N, S, D], w [D] or [D, 1], b [1], differentiable in all three."""
    N, S, _ = h.shape
    Sn = np.full(N, S, np.int64) if steps is None else np.asarray(steps, np.int64)
    y = torch.tensor(targets(Sn, S), dtype=h.dtype)
    z = h @ w.reshape(-1) + b.reshape(())
    sp = torch.nn.functional.softplus
    return (pos_weight * y * sp(-z) + (1.0 - y) * sp(z)).sum() / (N * S)
