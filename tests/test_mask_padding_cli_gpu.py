"""train.py with --hparams mask_padding=true on the tiny synthetic corpus of tests/test_guided_attn_cli_gpu.py: the feeder's
frame counts reach the masked losses through both loops, events.jsonl keeps its keys and carries finite (masked) losses,
and the one warning line appears exactly when nothing teaches the model where to stop."""
import numpy as np
import pytest

from test_guided_attn_cli_gpu import SMALL, _train

pytestmark = pytest.mark.gpu
WARNING = "mask_padding=true without stop_token=true"


def _check(r, ev, logged, steps):
    assert "mask_padding: True" in r.stdout
    assert sorted(logged) == list(range(1, steps + 1))
    assert ev
    for e in ev:
        assert {"loss", "loss_mel", "loss_linear"} <= set(e)
        assert all(np.isfinite(e[k]) and e[k] > 0.0 for k in ("loss", "loss_mel", "loss_linear")), e
        assert abs(logged[e["step"]] - e["loss"]) < 1e-5 + 1e-9, (logged, e["loss"])       # the line prints five decimals


def test_taco2_trains_with_the_switch_and_a_stop_token(tmp_path):
    # summaries at steps 2 and 4 (synchronous steps), steps 1 and 3 through the pipelined loop
    r, ev, logged = _train(tmp_path, "taco2", SMALL + ",mask_padding=true,stop_token=true", "fp32", 4, 2)
    assert [e["step"] for e in ev] == [2, 4]
    _check(r, ev, logged, 4)
    assert WARNING not in r.stdout + r.stderr
    for e in ev:
        assert abs(e["loss"] - (e["loss_mel"] + e["loss_linear"] + e["loss_stop"])) < 1e-9, e


def test_taco2_warns_without_a_stop_token(tmp_path):
    r, ev, logged = _train(tmp_path, "taco2", SMALL + ",mask_padding=true", "fp32", 2, 1)
    _check(r, ev, logged, 2)
    assert r.stdout.count(WARNING) == 1
    for e in ev:
        assert abs(e["loss"] - (e["loss_mel"] + e["loss_linear"])) < 1e-9, e


def test_taco1_trains_with_the_switch_and_warns(tmp_path):
    hps = "batch_size=2,batch_group_size=2,outputs_per_step=5,max_iters=12,mask_padding=true"
    r, ev, logged = _train(tmp_path, "taco1", hps, "mixed", 2, 1)
    _check(r, ev, logged, 2)
    assert r.stdout.count(WARNING) == 1
