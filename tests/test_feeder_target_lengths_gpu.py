"""target_lengths through the device side of the feeder: batches assembled in HBM (prepare_batch_device, the HBM-resident
feature cache) and batches staged through pinned memory, each behind a DeviceStager, with and without the prefetch
thread.  The frame count of row i must be where that row's features end."""
import os

import numpy as np
import pytest
import torch

from nspeech_amd import hparams as hparams_mod
from test_guided_attn_cli_gpu import _corpus

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device_cache", [True, False])
@pytest.mark.parametrize("prefetch", [False, True])
def test_stager_carries_the_frame_counts_of_its_batch(dev, tmp_path, device_cache, prefetch):
    from nspeech_amd.datasets.datafeeder import DataFeeder, DeviceStager
    data = str(tmp_path / "lj")
    os.makedirs(data)
    _corpus(data)
    hp = hparams_mod.load("taco2")
    hp.batch_size, hp.batch_group_size = 2, 2
    feeder = DataFeeder(hp, ljspeech=data, seed=7, prefetch=prefetch, pinned=not device_cache, device_cache=device_cache)
    stager = DeviceStager(feeder, "cuda:0")
    try:
        seen = set()
        for _ in range(4):
            inputs, lengths, mel, lin = stager.next_batch()          # the stager has already staged the batch AFTER this one
            tl = stager.target_lengths
            assert isinstance(tl, np.ndarray) and tl.dtype == np.int32 and tl.shape == (2,)
            assert torch.is_tensor(lin) and lin.is_cuda and lin.shape[1] > int(tl.max()) and lin.shape[1] % hp.outputs_per_step == 0
            torch.cuda.synchronize()
            for i in range(2):
                assert not bool(lin[i, tl[i]:].any()) and not bool(mel[i, tl[i]:].any())     # padding from there on
                assert bool(lin[i, tl[i] - 1].any())                                          # the last frame is real
            seen.update(int(t) for t in tl)
        assert len(seen) >= 3       # the four utterances differ in length: the counts follow the rows, not a constant
    finally:
        feeder.stop()
