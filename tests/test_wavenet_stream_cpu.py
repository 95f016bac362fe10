"""The host side of the resumable WaveNet generator (ns_wavenet_generate_span, include/nspeech_hip.h): the struct and the
entry point, the launcher's refusals (all before any launch, so the pointers below are never followed), safe_prefix -
what a streamed synthesis may hand out before the end point is known - against audio.find_endpoint itself, and
generate_wavenet.py's routing of --stream_chunk.  No device."""
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
    sp = _lib.struct("ns_wavenet_span_params")
    assert [f[0] for f in sp._fields_] == ["t_begin", "t_end", "carry"]
    kinds = dict(sp._fields_)
    assert kinds["t_begin"] is ctypes.c_int64 and kinds["t_end"] is ctypes.c_int64 and kinds["carry"] is ctypes.c_void_p
    assert "ns_wavenet_generate_span" in _lib.FUNCS and hasattr(_lib.lib(), "ns_wavenet_generate_span")
    assert "ns_wavenet_generate_span(const ns_wavenet_generate_params* p, const ns_wavenet_stop_params* stop," in open(_lib.HEADER_PATH).read()
    assert _lib.lib().ns_version() >= 106
    # the two older structs are what they were: cond_t0 last in 248 bytes, the stop's four members
    p = _lib.struct("ns_wavenet_generate_params")
    assert p._fields_[-1][0] == "cond_t0" and ctypes.sizeof(p) == 248
    assert [f[0] for f in _lib.struct("ns_wavenet_stop_params")._fields_] == ["below", "window", "hop", "end"]


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


def _span(t_begin, t_end, carry=0x1000):
    sp = _lib.struct("ns_wavenet_span_params")
    sp.t_begin, sp.t_end, sp.carry = t_begin, t_end, carry
    return sp


def _refused(p, st, sp):
    lib = _lib.lib()
    rc = lib.ns_wavenet_generate_span(ctypes.byref(p), ctypes.byref(st) if st is not None else None, ctypes.byref(sp), None)
    return rc, lib.ns_last_error().decode()


# every route of the launcher refuses in front of its own first launch: the per-layer kernel, the single-wave chain
# (engine 1), the MFMA chain without and with conditions (engine 2)
ROUTES = [dict(), dict(fgT=0x1000, deT=0x1000, engine=1), dict(fgT=0x1000, deT=0x1000, engine=2),
          dict(fgT=0x1000, deT=0x1000, engine=2, cond=0x1000)]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("t_begin,t_end", [(0, 5), (-3, 5), (5, 5), (7, 5), (1, 21), (20, 21), (1 << 32 | 1, 1 << 32 | 5)])
def test_bounds_outside_the_loop_are_refused(route, t_begin, t_end):
    for st in (None, _stop()):
        rc, msg = _refused(_params(**route), st, _span(t_begin, t_end))
        assert rc == ERR_ARG and msg.startswith("ns_wavenet_generate_span:") and "t_begin" in msg, msg


@pytest.mark.parametrize("route", ROUTES)
def test_a_stop_needs_a_carry(route):
    rc, msg = _refused(_params(**route), _stop(), _span(1, 20, carry=None))
    assert rc == ERR_ARG and msg.startswith("ns_wavenet_generate_span:") and "carry" in msg, msg
    rc, msg = _refused(_params(**route), _stop(), _span(5, 9, carry=None))
    assert rc == ERR_ARG and msg.startswith("ns_wavenet_generate_span:") and "carry" in msg, msg


def test_engine_3_takes_no_span():
    # everything engine 3 asks for is there (as far as a host check can tell): the span alone is refused, in front of the
    # clearing of post_x and the launch - even the span of the whole loop
    for sp in (_span(1, 20), _span(5, 9), _span(1, 20, carry=None)):
        rc, msg = _refused(_params(fgT=0x1000, deT=0x1000, engine=3, S=512, Q=256, post_x=0x1000, helper_stream=0x2000), None, sp)
        assert rc == ERR_ARG and msg.startswith("ns_wavenet_generate_span:") and "engine 3" in msg, msg


def test_the_plain_calls_refusals_come_first_and_unchanged():
    lib = _lib.lib()
    bad = _span(0, 99, carry=None)
    # ns_wavenet_generate's own
    for over, text in ((dict(cond=0x1000, fgT=0x1000, deT=0x1000, engine=1), "ns_wavenet_generate: conditions / biases"),
                       (dict(ids=None), "ns_wavenet_generate: null"), (dict(n_seed=1), "ns_wavenet_generate: bad sizes"),
                       (dict(temperature=-1.0), "ns_wavenet_generate: temperature"),
                       (dict(fgT=0x1000, deT=0x1000, engine=2, R=16, Dc=16), "ns_wavenet_generate: the MFMA chain needs"),
                       (dict(Dc=1, R=1), "ns_wavenet_generate: the per-layer kernel needs an even Dc")):
        p = _params(**over)
        assert lib.ns_wavenet_generate(ctypes.byref(p), None) == ERR_ARG
        plain = lib.ns_last_error().decode()
        assert plain.startswith(text), plain
        rc, msg = _refused(p, None, bad)
        assert rc == ERR_ARG and msg == plain
        rc, msg = _refused(p, _stop(), bad)
        assert rc == ERR_ARG and msg == plain
    # ns_wavenet_generate_until's own
    for over, word in ((dict(end=None), "end"), (dict(below=65), "below"), (dict(hop=7), "hop")):
        p, st = _params(), _stop(**over)
        assert lib.ns_wavenet_generate_until(ctypes.byref(p), ctypes.byref(st), None) == ERR_ARG
        plain = lib.ns_last_error().decode()
        assert plain.startswith("ns_wavenet_generate_until:") and word in plain
        rc, msg = _refused(p, st, bad)
        assert rc == ERR_ARG and msg == plain
    p = _params(fgT=0x1000, deT=0x1000, engine=3, S=512, Q=256, post_x=0x1000, helper_stream=0x2000)
    rc, msg = _refused(p, _stop(), _span(1, 20))
    assert rc == ERR_ARG and msg.startswith("ns_wavenet_generate_until:") and "engine 3" in msg, msg


# ------------------------------------------------------------------ 2. safe_prefix
def online_end(codes, below, window, hop):
    """The kernels' form (csrc/wavenet.hip, gen_stop_step): one pass, a run-length counter, the first window to fire."""
    n, run = len(codes), 0
    for j, c in enumerate(codes):
        run = run + 1 if c < below else 0
        x = j + 1 - window
        if run >= window and x >= hop and x % hop == 0 and x < n - window:
            return x + hop, j + 1             # the end, and the samples drawn
    return n, n


def test_safe_prefix_is_what_it_says():
    from nspeech_amd.models.wavenet import safe_prefix
    codes = np.asarray([9, 9, 1, 9, 2, 3, 4], np.int32)
    assert safe_prefix(codes, 7, 5, 6, 2) == 7 - 3                 # a run of 3 silent codes, window - hop = 4
    assert safe_prefix(codes, 7, 5, 4, 2) == 7 - 2                 # the run is longer than window - hop = 2
    assert safe_prefix(codes[-4:], 7, 5, 6, 2) == 7 - 3            # the tail is enough
    assert safe_prefix(codes, 7, 0, 6, 2) == 7 and safe_prefix(codes, 7, 10, 6, 2) == 3
    assert safe_prefix(codes[:2], 2, 10, 6, 2) == 0                # fewer drawn than window - hop, all silent
    assert safe_prefix(codes, 7, 5, 3, 3) == 7                     # hop == window: a later window starts at `drawn` or behind
    assert safe_prefix(codes[:0], 0, 5, 6, 2) == 0


def test_safe_prefix_never_passes_find_endpoints_cut(monkeypatch):
    """Random code rows handed out sample by sample: at every prefix length d that the online rule reaches without firing,
    safe_prefix(d) is at most the cut find_endpoint makes on the finished row, it never shrinks, and the final flush - the
    end the rule reports - is that cut."""
    from nspeech_amd.models.wavenet import endpoint_code, mu_law_decode, safe_prefix
    from nspeech_amd.utils import audio
    rng = np.random.RandomState(12)
    Q = 64
    thr = np.power(10.0, -40 * 0.05)
    below = endpoint_code(Q, thr)
    fired = rows = held = 0
    for _ in range(1500):
        n, window = int(rng.randint(10, 61)), int(rng.randint(3, 10))
        hop = int(rng.randint(1, window + 1))
        silent = rng.rand(n) >= rng.uniform(0.0, 0.5)
        codes = np.where(silent, rng.randint(0, below, n), rng.randint(below, Q, n)).astype(np.int32)
        monkeypatch.setattr(audio, "endpoint_rule", lambda *a, _r=(window, hop, thr): _r)
        want = audio.find_endpoint(mu_law_decode(codes, Q))
        end, drawn = online_end(codes, below, window, hop)
        assert end == want
        out = 0
        for d in range(1, drawn + 1):
            if d == drawn and drawn < n:      # the rule fires with this sample: the flush takes over
                break
            safe = safe_prefix(codes[max(0, d - (window - hop)):d], d, below, window, hop)
            assert safe == safe_prefix(codes[:d], d, below, window, hop)
            assert 0 <= safe <= end, (codes.tolist(), window, hop, d, safe, end)
            assert safe >= out                # what was handed out stays handed out
            out = safe
        assert out <= end                     # the final flush hands out [out, end): it equals find_endpoint's cut
        rows += 1
        fired += drawn < n
        held += out < min(drawn, end)
    assert fired >= rows / 5 and rows - fired >= rows / 5, (fired, rows)
    assert held >= rows / 5                   # the holding back is exercised, not only rows that end loud


# ------------------------------------------------------------------ 3. generate_wavenet.py --stream_chunk
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


def test_stream_chunk_needs_the_incremental_generator_alone(monkeypatch):
    gw = _no_model(monkeypatch)
    with pytest.raises(ValueError, match="--stream_chunk"):
        gw.main(_args(stream_chunk=2, fast_generation=False))
    with pytest.raises(ValueError, match="--stream_chunk"):           # the full-window path at another temperature
        gw.main(_args(stream_chunk=2, temperature=0.8))
    with pytest.raises(ValueError, match="--stream_chunk N and --save_every"):
        gw.main(_args(stream_chunk=2, save_every=2))
    # --save_every keeps its refusal with --stop_at_endpoint, with and without the new flag
    with pytest.raises(ValueError, match="no --save_every"):
        gw.main(_args(stop_at_endpoint=True, save_every=2))
    # with the generator it passes the refusals and reaches the model - together with --stop_at_endpoint true as well
    for over in (dict(stream_chunk=2), dict(stream_chunk=2, stop_at_endpoint=True),
                 dict(stream_chunk=2, temperature=0.8, incremental_temperature=True), dict(stream_chunk=None, save_every=2)):
        with pytest.raises(AssertionError, match="a model was built"):
            gw.main(_args(**over))
