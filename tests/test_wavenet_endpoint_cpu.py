"""The host side of the WaveNet generator's own end point (ns_wavenet_generate_until, include/nspeech_hip.h): the struct
and the entry point, the launcher's refusals (all before any launch, so the pointers below are never followed),
audio.endpoint_rule, models.wavenet.endpoint_code, the kernels' online form of find_endpoint's rule restated on the host
against audio.find_endpoint itself, and generate_wavenet.py's routing of --stop_at_endpoint.  No device."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from nspeech_amd import _lib  # noqa: E402

ERR_ARG = -1


# ------------------------------------------------------------------ 1. the C ABI
def test_struct_function_and_version():
    st = _lib.struct("ns_wavenet_stop_params")
    assert [f[0] for f in st._fields_] == ["below", "window", "hop", "end"]
    kinds = dict(st._fields_)
    assert kinds["below"] is ctypes.c_int and kinds["window"] is ctypes.c_int64 and kinds["hop"] is ctypes.c_int64
    assert kinds["end"] is ctypes.c_void_p
    assert "ns_wavenet_generate_until" in _lib.FUNCS and hasattr(_lib.lib(), "ns_wavenet_generate_until")
    assert _lib.lib().ns_version() >= 105
    # ns_wavenet_generate_params is what it was: cond_t0 last, 248 bytes
    p = _lib.struct("ns_wavenet_generate_params")
    assert p._fields_[-1][0] == "cond_t0" and ctypes.sizeof(p) == 248


def _params(**over):
    p = _lib.struct("ns_wavenet_generate_params")
    fake = 0x1000                            # non-null; every case here is refused before a kernel could read it
    for f in ("weights", "ids", "queues", "uniform", "dilations"):
        setattr(p, f, fake)
    p.w_dtype = _lib.NS_BF16
    p.L, p.R, p.Dc, p.S, p.Q = 8, 32, 32, 64, 64
    p.B, p.n_seed, p.total, p.queue_rows = 1, 12, 20, 30
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _stop(**over):
    st = _lib.struct("ns_wavenet_stop_params")
    st.below, st.window, st.hop, st.end = 10, 6, 2, 0x1000
    for k, v in over.items():
        setattr(st, k, v)
    return st


def _refused(p, st):
    lib = _lib.lib()
    rc = lib.ns_wavenet_generate_until(ctypes.byref(p), ctypes.byref(st), None)
    return rc, lib.ns_last_error().decode()


@pytest.mark.parametrize("over,word", [(dict(end=None), "end"), (dict(below=-1), "below"), (dict(below=65), "below"),
                                       (dict(window=0), "window"), (dict(hop=0), "hop"), (dict(hop=7), "hop")])
def test_a_bad_stop_is_refused(over, word):
    rc, msg = _refused(_params(), _stop(**over))
    assert rc == ERR_ARG and msg.startswith("ns_wavenet_generate_until:") and word in msg, msg


def test_engine_3_takes_no_stop():
    # everything engine 3 asks for is there (as far as a host check can tell): the stop alone is refused, in front of the
    # clearing of post_x and the launch
    rc, msg = _refused(_params(fgT=0x1000, deT=0x1000, engine=3, S=512, Q=256, post_x=0x1000, helper_stream=0x2000), _stop())
    assert rc == ERR_ARG and msg.startswith("ns_wavenet_generate_until:") and "engine 3" in msg, msg


def test_the_plain_calls_refusals_come_first_and_unchanged():
    lib = _lib.lib()
    p = _params(cond=0x1000, fgT=0x1000, deT=0x1000, engine=1)
    assert lib.ns_wavenet_generate_until(ctypes.byref(p), None, None) == ERR_ARG         # stop == NULL: ns_wavenet_generate
    assert "conditions / biases" in lib.ns_last_error().decode()
    rc, msg = _refused(p, _stop())
    assert rc == ERR_ARG and "conditions / biases" in msg


# ------------------------------------------------------------------ 2. audio.endpoint_rule
def test_endpoint_rule_is_what_find_endpoint_uses():
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.utils import audio
    hp = hparams_mod.load("taco2")
    assert hp.sample_rate == 20000
    assert audio.endpoint_rule() == (16000, 4000, 10 ** -2.0)
    # 20000 * 0.00055 = 11 samples, a hop of int(11 / 4) = 2; -20 dB = 0.1
    w, h, thr = audio.endpoint_rule(threshold_db=-20, min_silence_sec=0.00055)
    assert (w, h) == (11, 2) and thr == np.power(10.0, -1.0)
    wav = np.ones(40, np.float32)
    wav[7:] = 0.05                            # windows at x = 2, 4, 6 hold a loud sample; x = 8 is the first silent one
    assert audio.find_endpoint(wav, -20, 0.00055) == 10
    wav[18] = 1.0                             # x = 8 .. 18 hold it: x = 20 is next
    assert audio.find_endpoint(wav, -20, 0.00055) == 22
    wav[28] = 1.0                             # x = 18 .. 28 hold it; x < 40 - 11 leaves no later window
    assert audio.find_endpoint(wav, -20, 0.00055) == 40


# ------------------------------------------------------------------ 3. endpoint_code and the online rule
@pytest.mark.parametrize("Q", [64, 256])
def test_endpoint_code_counts_the_codes_below_the_threshold(Q):
    from nspeech_amd.models.wavenet import endpoint_code, mu_law_decode
    thr = np.power(10.0, -40 * 0.05)
    brute = sum(1 for c in range(Q) if float(mu_law_decode(np.asarray([c]), Q)[0]) < thr)
    assert endpoint_code(Q, thr) == brute and 0 < brute < Q
    assert endpoint_code(Q, -2.0) == 0 and endpoint_code(Q, 2.0) == Q
    dec = mu_law_decode(np.arange(Q), Q)
    assert (np.diff(dec) > 0).all()


def test_endpoint_code_refuses_a_decode_that_is_not_increasing(monkeypatch):
    from nspeech_amd.models import wavenet as W
    real = W.mu_law_decode
    monkeypatch.setattr(W, "mu_law_decode", lambda ids, q: -real(ids, q))
    with pytest.raises(ValueError, match="not increasing"):
        W.endpoint_code(64, 0.01)


def online_end(codes, below, window, hop):
    """The kernels' form (csrc/wavenet.hip, gen_stop_step): one pass, a run-length counter, the first window to fire."""
    n, run = len(codes), 0
    for j, c in enumerate(codes):
        run = run + 1 if c < below else 0
        x = j + 1 - window
        if run >= window and x >= hop and x % hop == 0 and x < n - window:
            return x + hop, j + 1             # the end, and the samples drawn
    return n, n


def test_online_rule_is_find_endpoint_on_the_decoded_codes(monkeypatch):
    from nspeech_amd.models.wavenet import endpoint_code, mu_law_decode
    from nspeech_amd.utils import audio
    rng = np.random.RandomState(11)
    Q = 64
    thr = np.power(10.0, -40 * 0.05)
    below = endpoint_code(Q, thr)
    fired = rows = 0
    for _ in range(3000):
        n, window = int(rng.randint(10, 61)), int(rng.randint(3, 10))
        hop = int(rng.randint(1, window + 1))
        # between no loud sample and one in two, row by row: rows with and without a silent window both occur
        silent = rng.rand(n) >= rng.uniform(0.0, 0.5)
        codes = np.where(silent, rng.randint(0, below, n), rng.randint(below, Q, n)).astype(np.int32)
        monkeypatch.setattr(audio, "endpoint_rule", lambda *a, _r=(window, hop, thr): _r)
        want = audio.find_endpoint(mu_law_decode(codes, Q))
        end, drawn = online_end(codes, below, window, hop)
        assert end == want, (codes.tolist(), window, hop, end, want)
        assert drawn == (end - hop + window if end < n else n)     # (a fired end is x + hop < n - window + hop <= n)
        rows += 1
        fired += drawn < n
    assert fired >= rows / 5 and rows - fired >= rows / 5, (fired, rows)


# ------------------------------------------------------------------ 4. generate_wavenet.py --stop_at_endpoint
def _args(**over):
    a = dict(checkpoint="/nonexistent/model.ckpt-0", hparams="", gc_channels=None, lc_channels=None, local_condition=None, lc_hold=1,
             samples=4, fast_generation=True, temperature=1.0, precision="bf16", seed=0, wav_seed=None, save_every=None)
    a.update(over)
    return argparse.Namespace(**a)


def _no_model(monkeypatch):
    import generate_wavenet

    def refuse(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(generate_wavenet, "create_model", refuse)
    return generate_wavenet


def test_stop_at_endpoint_needs_the_incremental_generator(monkeypatch):
    gw = _no_model(monkeypatch)
    with pytest.raises(ValueError, match="--stop_at_endpoint"):
        gw.main(_args(stop_at_endpoint=True, fast_generation=False))
    with pytest.raises(ValueError, match="--stop_at_endpoint"):       # the full-window path at another temperature
        gw.main(_args(stop_at_endpoint=True, temperature=0.8))
    with pytest.raises(ValueError, match="--save_every"):
        gw.main(_args(stop_at_endpoint=True, save_every=2))
    # with the generator it passes the refusals and reaches the model; without the flag nothing changes
    for over in (dict(stop_at_endpoint=True), dict(stop_at_endpoint=True, temperature=0.8, incremental_temperature=True),
                 dict(stop_at_endpoint=False, fast_generation=False), dict(fast_generation=False)):
        with pytest.raises(AssertionError, match="a model was built"):
            gw.main(_args(**over))
