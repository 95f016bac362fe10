"""Placement of the persistent kernels' clusters (csrc/exchange.h, ns_cluster_place): with NS_CLUSTER_XCD=1 the workgroups
of a cluster share one residue of the grid index mod 8 - one XCD under round-robin dispatch - and with NS_CLUSTER_XCD=0
they are dealt b / members, b % members.  Only which CU runs which role moves, so every output and history buffer must
hold the SAME BITS either way - torch.equal, no tolerance - with the status words 0 after every launch.  The shapes are
the smallest that reach a padded grid (clusters % 8 != 0), two slots on one XCD (clusters > 8) and each rows-per-chain
form.  The probe at the end checks on the device that a placed cluster does sit on one XCD."""
import pytest
import torch

from test_gru_seq_gpu import _case as _gru_case
from test_lstm_cluster_lanes_gpu import KEYS as LSTM_KEYS, _data as _lstm_data, _run as _lstm_run
from test_lstm_cluster_rows_gpu import _fp32_data, _run_fp32
from util import make_batch, small_hparams

pytestmark = pytest.mark.gpu

MODES = (("1", "placed"), ("0", "linear"))


def _both(monkeypatch, run):
    """run() under NS_CLUSTER_XCD=1, then under NS_CLUSTER_XCD=0"""
    out = []
    for value, _ in MODES:
        monkeypatch.setenv("NS_CLUSTER_XCD", value)
        out.append(run())
    return out


def _same(placed, linear, keys, what):
    for k in keys:
        assert placed[k].float().abs().max().item() > 0, (what, k, "nothing written")
        assert torch.equal(placed[k], linear[k]), (what, k, (placed[k].float() - linear[k].float()).abs().max().item())


# BiLSTM clusters (lstm_cluster2_fwd / lstm_cluster2p_bwd): H 64 = one workgroup per chain, H 256 = four.
#   N 5 at 4 rows: 4 chains - a padded grid;  N 32 at 4 rows: 16 chains - two slots per XCD;  N 3 at 8 and at 16 rows:
#   2 chains, the other two forms.  _lstm_run asserts the status word and the form after every launch.
@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("N,T,rows", [(5, 6, 4), (32, 6, 4), (3, 5, 8), (3, 5, 16)])
def test_bilstm_clusters_bit_equal(dev, monkeypatch, N, T, rows, H):
    monkeypatch.delenv("NS_CLUSTER_DBG", raising=False)
    monkeypatch.setenv("NS_CLUSTER_ROWS", str(rows))
    data = _lstm_data(dev, N, T, H, lengths="random")
    placed, linear = _both(monkeypatch, lambda: _lstm_run(dev, data, rows))
    _same(placed, linear, LSTM_KEYS, (N, T, rows, H))


def test_bilstm_fp32_state_forward_bit_equal(dev, monkeypatch):
    """lstm_cluster3_fwd at N 5, T 6, H 64: 4 chains of two workgroups at 4 rows, a padded grid"""
    monkeypatch.delenv("NS_CLUSTER_DBG", raising=False)
    monkeypatch.setenv("NS_CLUSTER_ROWS", "4")
    data = _fp32_data(dev, 5, 6, 64, True)
    (placed, pf), (linear, lf) = _both(monkeypatch, lambda: _run_fp32(dev, data))       # (the status word: _run_fp32)
    assert pf == [4] and lf == [4], (pf, lf)
    _same(placed, linear, ("h", "hb", "c_fw", "c_bw", "g_fw", "g_bw"), "fp32 state")


# Attention clusters (attn_cluster_fwd / attn_cluster_bwd), 8 workgroups per utterance, T_in 24, 4 decoder steps:
#   N 3: a padded grid (64 indices, 24 active);  N 9: padded, utterances 0 and 8 in two slots of one XCD
ATTN_HIST = ("dec_p1", "dec_xa", "dec_hc", "dec_ca", "dec_ga", "dec_q", "dec_al", "dec_al_t")
ATTN_GRAD = ("d_f1", "d_p2", "d_ga", "d_q", "d_energy", "d_keys", "d_values", "d_wcl")


@pytest.mark.parametrize("mode", ["fp32", "mixed"])
@pytest.mark.parametrize("N", [3, 9])
def test_attention_clusters_bit_equal(dev, monkeypatch, N, mode):
    from nspeech_amd.models import create_model
    hp = small_hparams()
    m = create_model("taco2", hp, device="cuda:0", dtype=mode, seed=3)
    m.use_attn_cluster = True
    m.deterministic = True
    m.overlap_wgrads = False            # one stream: every buffer has its final contents when the pass returns
    inputs, lengths, mel, lin = make_batch(hp, N, 24, 4 * hp.outputs_per_step, seed=N)

    def run():
        m.initialize(inputs, lengths, None, mel, lin)
        assert m._attn_cluster_fwd, "the cluster kernel must cover this shape"
        m.backward()
        torch.cuda.synchronize()
        m.check_status()                # every status word of the pass
        assert m.last_paths["attn:fwd"] == "cluster" and m.last_paths["attn:bwd"] == "cluster", m.last_paths
        out = {k: m._bufs[k].clone() for k in ATTN_HIST + ATTN_GRAD}
        out["flat_g"] = m.flat_g.clone()
        return out

    placed, linear = _both(monkeypatch, run)
    _same(placed, linear, ATTN_HIST + ATTN_GRAD + ("flat_g",), (N, mode))


def test_gru256_clusters_bit_equal(dev, monkeypatch):
    """gru_fwd / gru_bwd at H 256 (4 workgroups per chain), N 3, T 5, two directions: 2 chains, a padded grid.  The
    harness of test_gru_seq_gpu.py checks the status word after each direction's launches."""
    placed, linear = _both(monkeypatch, lambda: _gru_case(dev, 3, 5, 256, 2, True, True, "fp32", 3, seed=8))
    for (p, _), (q, _) in zip(placed, linear):
        _same(p, q, ("h", "ru", "c", "rh", "dzg", "dzc", "dh0"), "gru")


TACO1_HIST = ("dec_p1", "dec_xa", "dec_xc", "dec_hc", "dec_ru", "dec_cc", "dec_q", "dec_al", "dec_al_t")
TACO1_GRAD = ("att_dzg", "att_dzc", "att_dp2", "att_df1", "att_dq", "att_de")


def test_taco1_attention_clusters_bit_equal(dev, monkeypatch):
    """taco1_attn_fwd / taco1_attn_bwd (8 workgroups per utterance) at N 3, inside a training pass at the shipped widths
    (the kernels exist for A = 256 only); the residual GRU(256) clusters of the decoder run in the same pass."""
    from nspeech_amd import hparams as hparams_mod
    from nspeech_amd.models import create_model
    hp = hparams_mod.load("taco1")
    m = create_model("taco1", hp, device="cuda:0", dtype="fp32", seed=3)
    m.deterministic = True
    inputs, lengths, mel, lin = make_batch(hp, 3, 12, 4 * hp.outputs_per_step, seed=11)

    def run():
        m.initialize(inputs, lengths, None, mel, lin)
        m.backward()
        torch.cuda.synchronize()
        m.check_status()
        assert m.last_paths["attn:fwd"] == "cluster" and m.last_paths["attn:bwd"] == "cluster", m.last_paths
        out = {k: m._bufs[k].clone() for k in TACO1_HIST + TACO1_GRAD}
        out.update(mel=m.mel_outputs.clone(), lin=m.linear_outputs.clone(), align=m.alignments.clone())
        return out

    placed, linear = _both(monkeypatch, run)
    _same(placed, linear, TACO1_HIST + TACO1_GRAD + ("mel", "lin", "align"), "taco1")


# ------------------------------------------------------------------ where the workgroups run
def _probe(dev, clusters, members, placed):
    import ctypes
    from nspeech_amd import _lib, ops
    xcc = torch.full((clusters * members,), -1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().ns_cluster_probe(clusters, members, int(placed), ctypes.c_void_p(xcc.data_ptr()),
                                           ctypes.c_void_p(ops.stream())), "ns_cluster_probe")
    torch.cuda.synchronize()
    ids = xcc.cpu().tolist()
    assert all(0 <= i < 8 for i in ids), ids             # every active workgroup reported
    return ids


@pytest.mark.parametrize("clusters", [16, 5])
def test_placed_clusters_sit_on_one_xcd(dev, clusters):
    members = 4
    linear = _probe(dev, clusters, members, False)       # linear: the report of grid index b is linear[b]
    print("clusters %d linear %s" % (clusters, linear))
    premise = all(linear[b] == linear[b + 8] for b in range(len(linear) - 8)) and \
        all(len(set(linear[b:b + 8])) == 8 for b in range(0, len(linear) - 7, 8))
    if not premise:
        pytest.skip("index b and b + 8 do not share an XCD, or eight consecutive indices do not cover eight XCDs, "
                    "in a linear launch: this machine deals workgroups differently, which costs speed, not correctness")
    placed = _probe(dev, clusters, members, True)
    print("clusters %d placed %s" % (clusters, placed))
    for c in range(clusters):
        ids = set(placed[c * members:(c + 1) * members])
        assert len(ids) == 1, (c, placed)
