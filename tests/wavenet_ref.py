"""Float64 contract of csrc/wavenet.hip and of the WaveNet models' arrangements (models/wavenet.py), on the CPU.  TEST
INFRASTRUCTURE ONLY; imports nothing from nspeech_amd.  tests/test_wavenet_ref_cpu.py proves it (against
oracle/wavenet_oracle.py, scalar loops and autograd), tests/test_wavenet_contract_gpu.py holds the kernels to it.

The pieces restate their comments in include/nspeech_hip.h: input_fwd / input_bwd, gate_fwd / gate_bwd, softmax_ce,
softmax64.

The network (ids [N, T0] -> logits at every position t >= rf - 1) takes a PRESET = the set of rounding points of an
arrangement, read off the kernels.  bf16 = round to nearest even through torch.bfloat16.
  pure     nothing is rounded: oracle.wavenet_oracle.network / network_full.
  w_bf16   the per-layer generator on the bf16 shadow (wn_generate_kernel<bf16_t>) and engine 1
           (wn_generate_fast_kernel): "w" - every weight is bf16, the causal table included, and so are the condition
           vectors (embedding row, local condition rows) and kernels, which models/wavenet.py:_generator_terms multiplies
           in the weights' dtype.  Activations, the rings, the skip and post-processing sums are fp32 and never rounded;
           the condition TERMS and all biases are fp32 addends.
  mfma     engines 2 and 3 (wn_generate_mfma_kernel): "w", and
           "fg_operand"    both operands of the filter | gate product, x[t - d] (from the ring) and x[t], are rounded
                           where the product reads them (mf_pack): the ring and the residual keep the fp32 values;
           "dense_operand" the gated output is rounded as the operand of the dense product only (b_out); the skip waves
                           read the unrounded value from LDS.
           Dense, skip and post biases and the condition terms are fp32 addends.
  train_bf16  the bf16 training pass of models/wavenet.py (train() below, forward and a hand-written backward): the
           buffers xs, outs, t1, c1, dlogits, dp1, dsk, douts, dout_l, dz, dx, dx_tmp are stored as bf16 (a value is rounded
           once, where it is stored); zs, logits, dc1, dt1, the held condition's term and its gradient, and the weight
           gradients are fp32.  Products follow tests/gemm_ref.py's rule: exact products of the stored operands, bias and
           addend added unrounded, one rounding at the store.  "w": the kernels are the bf16 shadow as every product's
           B operand; the biases and the causal table (ns_wavenet_input reads the fp32 master) are not rounded.
           "frames": the held condition's frames are rounded once (both products that read them see those values).
Because the rings hold unrounded x and every rounding happens at use, the sliding-window network with these hooks IS the
incremental generator's contract, and one pass over a finished waveform gives the distribution behind every draw.

generate() is the free run with the kernels' draw rule: uniforms rounded to float32 (as model.generate does), float64
softmax weights ex = exp(logit - max), the first class j with u * sum(ex) < ex[0] + .. + ex[j], the last class otherwise.
safe_uniforms() draws the uniforms of a case: numpy's Generator(seed), where a number that falls within `delta` of a
CDF edge OF THE REFERENCE is drawn again from the same stream.  With delta = 2 x the case's CDF bound a kernel within
its bound reproduces the reference's run exactly (cdf_margin() measures what a run was left with).

PLANTS: mistakes the contract must reject, switched on by plant= (the CPU module shows every GPU case's tolerances
reject each where it applies)."""
import numpy as np
import torch

f64 = torch.float64
PRESETS = {
    "pure": frozenset(),
    "w_bf16": frozenset({"w"}),
    "mfma": frozenset({"w", "fg_operand", "dense_operand"}),
    "train_bf16": frozenset({"w", "frames", "xs", "outs", "t1", "c1", "dlogits", "dp1", "dsk", "douts", "dout_l", "dz", "dx", "dx_tmp"}),
}
NET_PRESETS = ("pure", "w_bf16", "mfma")          # the generator's arrangements (network()); train_bf16 is train()'s
NET_PLANTS = ("skip_last", "skip_mid", "ring_slot", "taps_swapped", "dense_ahead", "out_unrounded", "residual_rounded",
              "dense_bias_64", "cond_row", "cond_halves", "uniform_index", "causal_swapped")
PIECE_PLANTS = ("gate_bwd_filter", "ce_no_onehot", "input_bwd_start")


def bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def dilations(hp):
    return [2 ** i for _ in range(hp["dilations_depth"]) for i in range(hp["dilations_length"])]


def receptive_field(hp):
    return sum(dilations(hp)) + 2


# ------------------------------------------------------------------------------------------------------------ the pieces
def input_fwd(ids, w):
    """x[n, t, :] = w[0][ids[n, t-1]] + w[1][ids[n, t]] for t >= 1; row t = 0 is zero.  ids [N, T], w [2, Q, C]."""
    ids = ids.long()
    x = torch.zeros(ids.shape[0], ids.shape[1], w.shape[2], dtype=w.dtype)
    x[:, 1:] = w[0][ids[:, :-1]] + w[1][ids[:, 1:]]
    return x


def input_bwd(ids, dx, dw, start=0, plant=None):
    """dw[0][ids[t-1]] += dx[t], dw[1][ids[t]] += dx[t] for t >= max(1, start).  Returns dw + the sums (dw [2, Q, C])."""
    ids = ids.long()
    s = max(1, start) if plant != "input_bwd_start" else max(1, start - 1)
    out = dw.clone().double()
    C = dw.shape[2]
    g = dx.double()[:, s:].reshape(-1, C)
    out[0].index_add_(0, ids[:, s - 1:-1].reshape(-1), g)
    out[1].index_add_(0, ids[:, s:].reshape(-1), g)
    return out


def hold_rows(T, t0, hold, rows):
    """Condition row of positions 0 .. T-1: min(rows - 1, max(0, t + t0) // hold), t0 one int."""
    t = torch.arange(T, dtype=torch.long)
    return torch.clamp(torch.clamp(t + int(t0), min=0) // int(hold), max=rows - 1)


def _gate_pre(z, T, cond, hold, t0):
    """z [N*T, 2C] + the held condition term cond [N, rows, >= 2C] (t0 [N]) -> [N, T, 2C]."""
    twoC = z.shape[1]
    z = z.double().reshape(-1, T, twoC)
    if cond is not None:
        N, rows = cond.shape[0], cond.shape[1]
        idx = torch.stack([hold_rows(T, int(t0[n]), hold, rows) for n in range(N)])
        z = z + torch.stack([cond[n, idx[n], :twoC].double() for n in range(N)])
    return z


def gate_fwd(z, T, start, cond=None, hold=1, t0=None):
    """out [N*T, C] = tanh(zf) * sigmoid(zg); rows with t < start are 0."""
    zz = _gate_pre(z, T, cond, hold, t0)
    C = zz.shape[2] // 2
    out = torch.tanh(zz[..., :C]) * torch.sigmoid(zz[..., C:])
    out[:, :start] = 0
    return out.reshape(-1, C)


def gate_bwd(z, dout, T, start, cond=None, hold=1, t0=None, plant=None):
    """dz [N*T, 2C] = [dout sg (1 - th^2) | dout th sg (1 - sg)]; rows with t < start are 0."""
    zz = _gate_pre(z, T, cond, hold, t0)
    C = zz.shape[2] // 2
    th, sg = torch.tanh(zz[..., :C]), torch.sigmoid(zz[..., C:])
    g = dout.double().reshape(-1, T, C).clone()
    g[:, :start] = 0
    df = g * sg * (1 - th * th) if plant != "gate_bwd_filter" else g * sg * (1 - sg)
    return torch.cat([df, g * th * sg * (1 - sg)], dim=2).reshape(-1, 2 * C)


def softmax_ce(logits, targets, scale, plant=None):
    """(scale * sum_rows (logsumexp - logit[target]),  dlogits = scale * (softmax - onehot)); logits [rows, Q]."""
    lg = logits.double()
    lse = torch.logsumexp(lg, dim=1)
    tg = targets.long()
    loss = scale * (lse - lg.gather(1, tg[:, None])[:, 0]).sum()
    d = torch.softmax(lg, dim=1)
    if plant != "ce_no_onehot":
        d = d - torch.nn.functional.one_hot(tg, lg.shape[1]).double()
    return loss, scale * d


def softmax64(logits):
    return torch.softmax(logits.double(), dim=-1)


# ------------------------------------------------------------------------------------------------------------ the network
def param_shapes(hp):
    """The reference's variable names and shapes (neural_speech/models/wavenet.py:136-254), in creation order."""
    Q, R, Dc, S = hp["quantization_channels"], hp["residual_channels"], hp["dilation_channels"], hp["skip_channels"]
    gc, lc = hp.get("gc_channels") or 0, hp.get("lc_channels") or 0
    d = {}
    if gc and hp.get("gc_category_cardinality"):
        d["wavenet/embeddings/gc_embedding"] = (hp["gc_category_cardinality"], gc)
    d["wavenet/causal_layer/filter"] = (2, Q, R)
    for i in range(len(dilations(hp))):
        pre = "wavenet/dilated_stack/layer%d/" % i
        d[pre + "filter"], d[pre + "gate"] = (2, R, Dc), (2, R, Dc)
        d[pre + "dense"], d[pre + "skip"] = (1, Dc, R), (1, Dc, S)
        if gc:
            d[pre + "gc_gate"], d[pre + "gc_filter"] = (1, gc, Dc), (1, gc, Dc)
        if lc:
            d[pre + "lc_gate"], d[pre + "lc_filter"] = (1, lc, Dc), (1, lc, Dc)
        if hp["use_biases"]:
            d[pre + "filter_bias"], d[pre + "gate_bias"] = (Dc,), (Dc,)
            d[pre + "dense_bias"], d[pre + "slip_bias"] = (R,), (S,)
    d["wavenet/postprocessing/postprocess1"] = (1, S, S)
    d["wavenet/postprocessing/postprocess2"] = (1, S, Q)
    if hp["use_biases"]:
        d["wavenet/postprocessing/postprocess1_bias"] = (S,)
        d["wavenet/postprocessing/postprocess2_bias"] = (Q,)
    return d


def init_params(hp, seed, sharpen=None, causal_gain=None, dense_gain=None, bias_scale=0.3, cond_scale=1.0):
    """float32 numpy values for every variable: Glorot-uniform kernels (fans as tf's conv2d initialiser counts them),
    biases randn * bias_scale and the embedding randn * cond_scale - so that a bias on the wrong tensor shows.  Three
    gains by depth L shape the distributions so that a case can be decided at all: every draw's largest probability above
    4 / Q (structure), and few enough classes of weight that uniform numbers exist 2 x the CDF bound away from every edge.
      causal table x 8 (x 4 at 8 <= L < 16): activations of order 1 from the first layer on;
      postprocess2 x 10 as the existing generator tests do, x 20 with fewer than five layers and x 40 with fewer than
      three, whose skip sums are small, and x 4 at Q = 256 below 16 layers, where a probability is a quarter as large;
      dense kernels x 1/8 at L >= 16: with Glorot-sized residual updates 66 layers amplify one bf16 step of one value to
      a tenth of the CDF, and no margin could hold."""
    L = len(dilations(hp))
    if sharpen is None:
        sharpen = 40.0 if L < 3 else 20.0 if L < 5 else 10.0
        if hp["quantization_channels"] >= 256 and L < 16:
            sharpen *= 4.0
    if causal_gain is None:
        causal_gain = 4.0 if 8 <= L < 16 else 8.0
    if dense_gain is None:
        dense_gain = 0.125 if L >= 16 else 1.0
    rng = np.random.RandomState(seed)
    out = {}
    for k, shp in param_shapes(hp).items():
        if k.endswith("_bias"):
            out[k] = (rng.randn(*shp) * bias_scale).astype(np.float32)
        elif k.endswith("gc_embedding"):
            out[k] = (rng.randn(*shp) * cond_scale).astype(np.float32)
        else:
            rec = int(np.prod(shp[:-2]))
            lim = np.sqrt(6.0 / (rec * shp[-2] + rec * shp[-1]))
            out[k] = rng.uniform(-lim, lim, size=shp).astype(np.float32)
    out["wavenet/postprocessing/postprocess2"] = out["wavenet/postprocessing/postprocess2"] * np.float32(sharpen)
    out["wavenet/causal_layer/filter"] = out["wavenet/causal_layer/filter"] * np.float32(causal_gain)
    for k in out:
        if k.endswith("/dense"):
            out[k] = out[k] * np.float32(dense_gain)
    return out


def as_params(p, dtype=f64):
    return {k: torch.as_tensor(np.asarray(v), dtype=dtype) if not torch.is_tensor(v) else v.to(dtype) for k, v in p.items()}


def cond_terms(p, hp, preset="pure", gc=None, lc=None):
    """What joins a layer's [filter | gate] pre-activations besides the convolution, [N, rows, L, 2Dc] or None:
    embedding row (gc: [N] category ids) . [gc_filter | gc_gate] + [filter_bias | gate_bias] on every row, plus row r's
    own lc[n, r] . [lc_filter | lc_gate] (lc [N, rows, lc_channels]).  With "w" vectors and kernels are bf16, biases not."""
    r = PRESETS[preset]
    rw = bf16 if "w" in r else (lambda v: v)
    L = len(dilations(hp))
    if gc is None and lc is None and not hp["use_biases"]:
        return None
    N = len(gc) if gc is not None else (lc.shape[0] if lc is not None else 1)          # biases alone: one row for all
    rows = lc.shape[1] if lc is not None else 1
    Dc = hp["dilation_channels"]
    out = torch.zeros(N, rows, L, 2 * Dc, dtype=f64)
    for l in range(L):
        pre = "wavenet/dilated_stack/layer%d/" % l
        if gc is not None:
            h = rw(p["wavenet/embeddings/gc_embedding"].double()[torch.as_tensor(gc).long()])
            out[:, :, l] += (h @ rw(torch.cat([p[pre + "gc_filter"][0], p[pre + "gc_gate"][0]], dim=1).double()))[:, None]
        if hp["use_biases"]:
            out[:, :, l] += torch.cat([p[pre + "filter_bias"], p[pre + "gate_bias"]]).double()
        if lc is not None:
            c = rw(torch.as_tensor(lc, dtype=f64))
            out[:, :, l] += c @ rw(torch.cat([p[pre + "lc_filter"][0], p[pre + "lc_gate"][0]], dim=1).double())
    return out


def _flip_one(rounded, rows):
    """`rounded` with its largest-magnitude value on the last `rows` time positions moved one bf16 step up in magnitude."""
    v = rounded.clone()
    tail = v[:, -rows:]
    idx = np.unravel_index(int(tail.abs().argmax()), tuple(tail.shape))
    x = float(tail[idx])
    step = 2.0 ** (np.floor(np.log2(abs(x))) - 7) if x != 0 else 2.0 ** -133
    tail[idx] = x + (step if x >= 0 else -step)          # (a view of v)
    return v


def network(p, hp, ids, preset="pure", cond=None, hold=1, t0=0, pos0=0, dtype=f64, perm=None, plant=None, flip=None,
            flip_rows=1):
    """Logits [N, T0 - rf + 1, Q] of ids [N, T0] (the network's input; position i of it is position pos0 + i of the
    waveform the condition's time axis refers to).  cond: cond_terms(); the layer output at waveform position m takes row
    min(rows - 1, max(0, m + t0) // hold).  dtype / perm: the same arrangement in another float type with every product's
    K axis permuted (a float32 emulation that sums in another order).  flip = (layer, "x" | "out"): _flip_one at that
    rounding point.  p: float64 tensors by the reference's variable names."""
    r = PRESETS[preset]
    rw = (lambda v: bf16(v.double()).to(dtype)) if "w" in r else (lambda v: v.to(dtype))
    dil = dilations(hp)
    L, rf = len(dil), receptive_field(hp)
    bias = bool(hp["use_biases"])
    N, T0 = ids.shape
    ow = T0 - rf + 1
    assert ow >= 1

    def mm(a, w):
        if perm is None:
            return a @ w
        k = perm[w.shape[0]]
        return a[..., k] @ w[k]

    def rnd(v, point, l):
        if point not in r:
            return v
        out = bf16(v)
        if flip is not None and flip == (l, "x" if point == "fg_operand" else "out"):
            out = _flip_one(out, flip_rows)
        return out
    ids = ids.long()
    ct = rw(p["wavenet/causal_layer/filter"])
    if plant == "causal_swapped":
        ct = ct.flip(0)
    cur = ct[0][ids[:, :-1]] + ct[1][ids[:, 1:]]                        # positions 1 .. T0 - 1
    first = 1
    skips = 0
    for l, d in enumerate(dil):
        pre = "wavenet/dilated_stack/layer%d/" % l
        w = rw(torch.cat([p[pre + "filter"], p[pre + "gate"]], dim=2))   # [2, R, 2Dc]
        if plant == "taps_swapped":
            w = w.flip(0)
        xo = rnd(cur, "fg_operand", l)
        if plant == "residual_rounded":
            cur = bf16(cur)
        T = cur.shape[1] - d
        old = xo[:, :T] if not (plant == "ring_slot" and d > 1) else xo[:, 1:T + 1]
        z = mm(old, w[0]) + mm(xo[:, d:], w[1])
        first += d
        if cond is not None:
            rows = cond.shape[1]
            shift = 1 if plant == "cond_row" else 0
            idx = hold_rows(first + T + shift, t0 + pos0, hold, rows)[first + shift:]
            c = cond[:, idx, l].to(dtype)
            if plant == "cond_halves":
                c = torch.cat([c[..., c.shape[-1] // 2:], c[..., :c.shape[-1] // 2]], dim=-1)
            z = z + c
        Dc = z.shape[-1] // 2
        out = torch.tanh(z[..., :Dc]) * torch.sigmoid(z[..., Dc:])
        ld = l
        if plant == "dense_ahead" and l >= L - 2:
            ld = (l + 2) % L
        oo = rnd(out, "dense_operand", l) if plant != "out_unrounded" else out
        tr = mm(oo, rw(p["wavenet/dilated_stack/layer%d/dense" % ld][0]))
        sk = mm(out[:, T - ow:], rw(p[pre + "skip"][0]))
        if bias:
            if not (plant == "dense_bias_64" and l == 64):
                tr = tr + p[pre + "dense_bias"].to(dtype)
            sk = sk + p[pre + "slip_bias"].to(dtype)
        if (plant == "skip_last" and l == L - 1) or (plant == "skip_mid" and l == L // 2 and L > 1):
            sk = sk * 0 + (p[pre + "slip_bias"].to(dtype) if bias else 0)
        skips = skips + sk
        cur = cur[:, d:] + tr
    c1 = mm(torch.relu(skips), rw(p["wavenet/postprocessing/postprocess1"][0]))
    if bias:
        c1 = c1 + p["wavenet/postprocessing/postprocess1_bias"].to(dtype)
    c2 = mm(torch.relu(c1), rw(p["wavenet/postprocessing/postprocess2"][0]))
    if bias:
        c2 = c2 + p["wavenet/postprocessing/postprocess2_bias"].to(dtype)
    return c2


def plant_applies(plant, hp, preset, cond_rows):
    """Whether a planted error changes anything at this configuration."""
    dil = dilations(hp)
    L = len(dil)
    return {"skip_mid": L > 1, "ring_slot": max(dil) > 1, "dense_ahead": L > 2,
            # (nothing reads the last layer's dense product: at L = 1 neither its operand nor the residual matters)
            "out_unrounded": "dense_operand" in PRESETS[preset] and L > 1, "residual_rounded": L > 1,
            "dense_bias_64": L > 64 and bool(hp["use_biases"]), "cond_row": cond_rows > 1,
            "cond_halves": cond_rows >= 1}.get(plant, True)


def predict(p, hp, window, **kw):
    """Float64 softmax behind the last position of window [N, >= rf] -> [N, Q]."""
    return softmax64(network(p, hp, window, **kw)[:, -1])


def draw(pr_or_ex, u):
    """The kernels' draw rule on one row of softmax weights: the first j with u * sum < running sum, else the last."""
    c = np.cumsum(np.asarray(pr_or_ex, np.float64))
    return int(min(np.searchsorted(c, float(u) * c[-1], side="right"), len(c) - 1))


def edge_distance(pr, u):
    """Distance of u to the nearest inner edge of the CDF of pr (sum 1)."""
    c = np.cumsum(np.asarray(pr, np.float64))
    return float(np.abs(c[:-1] / c[-1] - float(u)).min())


def generate(p, hp, seeds, uniforms, plant=None, **kw):
    """Free run: seeds int [B, n_seed >= rf], uniforms [B, n] -> (ids [B, n_seed + n], probs [B, n, Q])."""
    rf = receptive_field(hp)
    wave = torch.as_tensor(np.asarray(seeds)).long()
    un = np.asarray(uniforms, np.float32)
    B, n = un.shape
    probs = []
    for i in range(n):
        T = wave.shape[1]
        pr = predict(p, hp, wave[:, T - rf:], pos0=T - rf, plant=plant, **kw)
        probs.append(pr)
        j = i if plant != "uniform_index" else (i + 1) % n
        nxt = [draw(pr[b].numpy(), un[b, j]) for b in range(B)]
        wave = torch.cat([wave, torch.tensor(nxt)[:, None]], dim=1)
    return wave.numpy().astype(np.int32), torch.stack(probs, dim=1)


def safe_uniforms(p, hp, seeds, n, seed, delta, **kw):
    """The uniforms [B, n] (float32) of a free run on the reference none of whose draws lies within delta of a CDF edge:
    numbers from numpy's Generator(seed), one that falls inside the band is drawn again from the same stream."""
    rng = np.random.default_rng(seed)
    rf = receptive_field(hp)
    wave = torch.as_tensor(np.asarray(seeds)).long()
    B = wave.shape[0]
    un = np.zeros((B, n), np.float32)
    for i in range(n):
        T = wave.shape[1]
        pr = predict(p, hp, wave[:, T - rf:], pos0=T - rf, **kw).numpy()
        nxt = []
        for b in range(B):
            for _ in range(1000):
                u = np.float32(rng.random())
                if edge_distance(pr[b], u) >= delta:
                    break
            else:
                raise AssertionError("no uniform number %g away from every CDF edge" % delta)
            un[b, i] = u
            nxt.append(draw(pr[b], u))
        wave = torch.cat([wave, torch.tensor(nxt)[:, None]], dim=1)
    return un


def cdf_margin(p, hp, seeds, uniforms, **kw):
    """The smallest distance, over the reference's free run, between a (float32) uniform number and a CDF edge."""
    ids, probs = generate(p, hp, seeds, uniforms, **kw)
    un = np.asarray(uniforms, np.float32)
    return min(edge_distance(probs[b, i].numpy(), un[b, i]) for b in range(un.shape[0]) for i in range(un.shape[1]))


def run_probs(p, hp, ids, n, **kw):
    """One pass over a finished waveform ids [B, total]: the distributions behind its last n samples, [B, n, Q]."""
    ids = torch.as_tensor(np.asarray(ids)).long()
    total = ids.shape[1]
    rf = receptive_field(hp)
    lo = total - n - rf                       # the window of the first of the n draws starts here
    return softmax64(network(p, hp, ids[:, lo:total - 1], pos0=lo, flip_rows=n, **kw))


class Perm(dict):
    """K-axis permutations by K for the float32 emulation, made when first asked for."""

    def __init__(self, seed=0):
        super().__init__()
        self.g = torch.Generator().manual_seed(seed)

    def __missing__(self, k):
        self[k] = torch.randperm(k, generator=self.g)
        return self[k]


# ------------------------------------------------------------------------------------------------------------ training
def train(p, hp, ids, preset="train_bf16", lc=None, hold=1, t0=None, dtype=f64, perm=None, flip=None):
    """The training pass of models/wavenet.py on ids [N, T] (mu-law codes of the clips), every series on ONE grid of
    T0 = T - 1 rows per item: logits [N, ow, Q], the mean cross-entropy and the gradient of every variable (by the
    reference's names), with the rounding points of `preset` (module docstring).  lc [N, F, lc_channels]: a held local
    condition, one frame per `hold` positions, t0 [N].  dtype / perm: the float32 emulation.  flip = (buffer, layer)."""
    r = PRESETS[preset]
    rw = (lambda v: bf16(v.double()).to(dtype)) if "w" in r else (lambda v: v.to(dtype))
    f_ = lambda v: v.to(dtype)                                            # noqa: E731  an fp32 master value
    dil = dilations(hp)
    L, rf = len(dil), receptive_field(hp)
    bias = bool(hp["use_biases"])
    ids = ids.long()
    net = ids[:, :-1]
    N, T0 = net.shape
    ow = T0 - rf + 1
    M = N * ow
    Dc = hp["dilation_channels"]
    starts = [1]
    for d in dil:
        starts.append(starts[-1] + d)

    def mm(a, w):
        if perm is None:
            return a @ w
        k = perm[w.shape[-2]]
        return a[..., k] @ w[..., k, :]

    def rd(v, name, l=None):
        if name not in r:
            return v
        out = bf16(v)
        if flip is not None and flip == (name, l):
            out = _flip_one(out, T0 - starts[l + 1] if name == "dz" else T0 - starts[l])
        return out

    def flat(v):
        return v.reshape(-1, v.shape[-1])
    pre = ["wavenet/dilated_stack/layer%d/" % l for l in range(L)]
    wfg = [rw(torch.cat([p[q + "filter"], p[q + "gate"]], dim=2)) for q in pre]
    wde = [rw(p[q + "dense"][0]) for q in pre]
    wsk = [rw(p[q + "skip"][0]) for q in pre]
    w1, w2 = rw(p["wavenet/postprocessing/postprocess1"][0]), rw(p["wavenet/postprocessing/postprocess2"][0])
    cterm = fr = idx = None
    if lc is not None:
        fr = rd(torch.as_tensor(lc, dtype=dtype), "frames")
        wlc = [rw(torch.cat([p[q + "lc_filter"][0], p[q + "lc_gate"][0]], dim=1)) for q in pre]
        cterm = [mm(fr, wlc[l]) for l in range(L)]                        # [N, F, 2Dc]
        idx = torch.stack([hold_rows(T0, int(t0[n]), hold, fr.shape[1]) for n in range(N)])
    # ---- forward
    xs = [rd(input_fwd(net, f_(p["wavenet/causal_layer/filter"])), "xs", 0)]
    zs, outs = [], []
    for l, d in enumerate(dil):
        x = xs[l]
        z = torch.zeros(N, T0, 2 * Dc, dtype=dtype)
        z[:, d:] = mm(x[:, :-d], wfg[l][0]) + mm(x[:, d:], wfg[l][1])
        if bias:
            z[:, d:] += f_(torch.cat([p[pre[l] + "filter_bias"], p[pre[l] + "gate_bias"]]))
        if cterm is not None:                   # joins inside the gate kernel: zs itself does not hold it
            z = z + torch.stack([cterm[l][n, idx[n]] for n in range(N)])
        zs.append(z)
        out = torch.tanh(z[..., :Dc]) * torch.sigmoid(z[..., Dc:])
        out[:, :starts[l + 1]] = 0
        out = rd(out, "outs", l)
        outs.append(out)
        xn = mm(out, wde[l]) + x
        if bias:
            xn = xn + f_(p[pre[l] + "dense_bias"])
        xs.append(rd(xn, "xs", l + 1))
    sk = sum(mm(outs[l][:, rf - 1:], wsk[l]) for l in range(L))
    if bias:
        sk = sk + sum(f_(p[q + "slip_bias"]) for q in pre)
    t1 = rd(torch.relu(sk), "t1")
    c1 = mm(t1, w1)
    if bias:
        c1 = c1 + f_(p["wavenet/postprocessing/postprocess1_bias"])
    c1 = rd(torch.relu(c1), "c1")
    logits = mm(c1, w2)
    if bias:
        logits = logits + f_(p["wavenet/postprocessing/postprocess2_bias"])
    loss, dl = softmax_ce(flat(logits), ids[:, rf:].reshape(-1), 1.0 / M)
    dl = rd(dl.to(dtype), "dlogits").reshape(N, ow, -1)
    # ---- backward
    g = {}
    g["wavenet/postprocessing/postprocess2"] = mm(flat(c1).t(), flat(dl))[None]
    dp1 = rd(mm(dl, w2.t()) * (c1 > 0), "dp1")
    g["wavenet/postprocessing/postprocess1"] = mm(flat(t1).t(), flat(dp1))[None]
    dsk = rd(mm(dp1, w1.t()) * (t1 > 0), "dsk")
    if bias:
        g["wavenet/postprocessing/postprocess2_bias"] = flat(dl).sum(0)
        g["wavenet/postprocessing/postprocess1_bias"] = flat(dp1).sum(0)
    dx = torch.zeros(N, T0, hp["residual_channels"], dtype=dtype)
    for l in range(L - 1, -1, -1):
        d, q = dil[l], pre[l]
        g[q + "skip"] = mm(flat(outs[l][:, rf - 1:]).t(), flat(dsk))[None]
        douts = torch.zeros(N, T0, Dc, dtype=dtype)
        douts[:, rf - 1:] = rd(mm(dsk, wsk[l].t()), "douts")
        dol = rd(mm(dx, wde[l].t()) + douts, "dout_l")
        g[q + "dense"] = mm(flat(outs[l]).t(), flat(dx))[None]
        if bias:
            g[q + "slip_bias"] = flat(dsk).sum(0)
            g[q + "dense_bias"] = flat(dx).sum(0)
        th, sg = torch.tanh(zs[l][..., :Dc]), torch.sigmoid(zs[l][..., Dc:])
        dol = dol.clone()
        dol[:, :starts[l + 1]] = 0
        dz = rd(torch.cat([dol * sg * (1 - th * th), dol * th * sg * (1 - sg)], dim=2), "dz", l)
        if bias:
            b = flat(dz).sum(0)
            g[q + "filter_bias"], g[q + "gate_bias"] = b[:Dc], b[Dc:]
        if fr is not None:
            dterm = torch.zeros(N, fr.shape[1], 2 * Dc, dtype=dtype)
            for n in range(N):
                dterm[n].index_add_(0, idx[n], dz[n])
            glc = mm(flat(fr).t(), flat(dterm))
            g[q + "lc_filter"], g[q + "lc_gate"] = glc[None, :, :Dc], glc[None, :, Dc:]
        g0 = mm(flat(xs[l][:, :-d]).t(), flat(dz[:, d:]))
        g1 = mm(flat(xs[l][:, d:]).t(), flat(dz[:, d:]))
        g[q + "filter"] = torch.stack([g0[:, :Dc], g1[:, :Dc]])
        g[q + "gate"] = torch.stack([g0[:, Dc:], g1[:, Dc:]])
        dxt = dx.clone()
        dxt[:, :-d] = dxt[:, :-d] + mm(dz[:, d:], wfg[l][0].t())
        dxt = rd(dxt, "dx_tmp")
        dx = rd(mm(dz, wfg[l][1].t()) + dxt, "dx")
    Q, R_ = hp["quantization_channels"], hp["residual_channels"]
    g["wavenet/causal_layer/filter"] = input_bwd(net, dx, torch.zeros(2, Q, R_, dtype=dtype), start=1).to(dtype)
    return dict(logits=logits, loss=loss, grads=g)
