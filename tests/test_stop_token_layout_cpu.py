"""hparam stop_token in the parameter layout: off = the layout as it was; on = two variables directly behind the output
projection's, inside the decoder bucket of the gradient reducer; out-of-range values are refused by the constructor."""
import pytest

from nspeech_amd import hparams as hparams_mod
from nspeech_amd import parallel
from nspeech_amd.models import params as P

from util import small_hparams

STOP = ("decoder/stop_projection/kernel", "decoder/stop_projection/bias")


def test_defaults_are_off_and_documented():
    hp = hparams_mod.load("taco2")
    assert hp.stop_token is False
    assert (hp.stop_token_weight, hp.stop_token_pos_weight, hp.stop_threshold) == (1.0, 1.0, 0.5)
    hp.parse("stop_token=true,stop_threshold=0.4,stop_token_pos_weight=5,stop_token_weight=0")
    assert hp.stop_token is True and hp.stop_threshold == 0.4 and hp.stop_token_pos_weight == 5.0
    assert hp.stop_token_weight == 0.0
    assert hparams_mod.load("taco1").stop_token is False


@pytest.mark.parametrize("full", [False, True])
def test_switch_off_is_the_layout_as_it_was(full):
    hp = hparams_mod.load("taco2") if full else small_hparams()
    tr, st = P.taco2_layout(hp, 149)
    assert not [k for k in tr.entries if "stop_projection" in k]
    tr_off, _ = P.taco2_layout(hp, 149, stop_token=False)
    assert list(tr.entries.items()) == list(tr_off.entries.items()) and tr.size == tr_off.size


@pytest.mark.parametrize("full", [False, True])
def test_switch_on_adds_two_variables_behind_the_output_projection(full):
    hp = hparams_mod.load("taco2") if full else small_hparams()
    off, st_off = P.taco2_layout(hp, 149)
    hp.stop_token = True
    on, st_on = P.taco2_layout(hp, 149)
    D = hp.decoder_lstm_units
    names = list(on.entries)
    i = names.index("decoder/output_projection/bias")
    assert tuple(names[i + 1:i + 3]) == STOP
    assert on.shape(STOP[0]) == (D, 1) and on.shape(STOP[1]) == (1,)
    assert [n for n in names if n not in STOP] == list(off.entries)
    assert list(st_on.entries.items()) == list(st_off.entries.items())
    # everything in front keeps its offset, everything behind moves by the two variables' padded sizes
    shift = on.off(names[i + 3]) - off.off(names[i + 3])
    assert shift == (D + 7) // 8 * 8 + 8 == on.size - off.size
    for n in off.entries:
        assert on.off(n) - off.off(n) == (0 if names.index(n) <= i else shift), n
    # the initial values: the kernel like every dense kernel, the bias zero
    pv, _ = P.init_values(on, st_on, seed=3)
    lim = (6.0 / (D + 1)) ** 0.5
    assert pv[STOP[0]].shape == (D, 1) and 0.0 < abs(pv[STOP[0]]).max() <= lim
    assert pv[STOP[1]].tolist() == [0.0]


def test_the_decoder_bucket_of_the_reducer_holds_them():
    hp = small_hparams(stop_token=True)
    tr, _ = P.taco2_layout(hp, 149)
    buckets = {name: (lo, hi) for name, lo, hi in parallel.bucket_ranges(tr)}
    lo, hi = buckets["decoder"]
    for n in STOP:
        assert lo <= tr.off(n) and tr.off(n) + tr.numel(n) <= hi
        for other, (a, b) in buckets.items():
            assert other == "decoder" or not (a <= tr.off(n) < b)
    assert sum(b - a for a, b in buckets.values()) == tr.size


class _NoDevice(Exception):
    pass


@pytest.mark.parametrize("over, word", [
    (dict(stop_token_weight=-0.1), "stop_token_weight"),
    (dict(stop_token_pos_weight=0.0), "stop_token_pos_weight"),
    (dict(stop_token_pos_weight=-2.0), "stop_token_pos_weight"),
    (dict(stop_threshold=0.0), "stop_threshold"),
    (dict(stop_threshold=1.0), "stop_threshold"),
    (dict(stop_token=True, decoder_lstm_units=96), "multiple of 64"),
])
def test_out_of_range_values_are_refused(over, word):
    """The constructor checks them before it touches the device, so this runs without one - with the switch off too."""
    from nspeech_amd.models import create_model
    with pytest.raises(ValueError, match=word):
        create_model("taco2", small_hparams(**over), device="cpu", dtype="fp32")


def test_tacotron1_refuses_the_switch():
    from nspeech_amd.models import create_model
    hp = hparams_mod.load("taco1")
    hp.stop_token = True
    with pytest.raises(ValueError, match="only the Tacotron-2 model"):
        create_model("taco1", hp, device="cpu", dtype="fp32")
