"""iSTFTNet generator on the CPU: the head's reference op against ``torch.istft`` in float64, the generator built
from ``config/hifigan/config_istft.json`` (hop, shapes, gradients, weight-norm folding, the config check), the
shipped HiFi-GAN config unchanged, the ``get_vocoder`` / training-CLI surface and the length-bucketed ``infer``."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "config", "hifigan", "config_istft.json")


def _istft_config():
    from speakingstyle_amd.models.hifigan import AttrDict

    with open(CFG) as f:
        return AttrDict(json.load(f))


def _torch_istft_head(x, w, b, n_fft=16, hop=4):
    """The construction the head is defined by: torch.istft(mag * e^{i phi}) of the conv of the reflect-padded rows."""
    a = F.leaky_relu(x, 0.01)
    p = torch.cat([a[:, 1:2], a], 1)
    z = F.conv1d(p.transpose(1, 2), w, b, padding=3)
    nb = n_fft // 2 + 1
    spec = torch.exp(z[:, :nb]) * torch.exp(1j * torch.sin(z[:, nb:]))
    return torch.istft(spec, n_fft, hop, n_fft, window=torch.hann_window(n_fft, dtype=x.dtype), center=True)


@pytest.mark.parametrize("T", [2, 3, 7, 64, 65, 130])
def test_reference_head_equals_torch_istft_float64(T):
    from speakingstyle_amd.ops import reference as ref

    torch.manual_seed(T)
    C = 128
    x = torch.randn(2, T, C, dtype=torch.float64)
    w = torch.randn(18, C, 7, dtype=torch.float64) * 0.02
    b = torch.randn(18, dtype=torch.float64) * 0.1
    y = ref.istft_head(x, w, b, 16, 4)
    want = _torch_istft_head(x, w, b)
    assert y.dtype == torch.float64 and y.shape == want.shape == (2, 4 * T)
    assert (y - want).abs().max().item() <= 1e-12
    one = ref.istft_head(x[0], w, b, 16, 4)  # one utterance without a batch axis
    assert one.shape == (4 * T,) and (one - want[0]).abs().max().item() <= 1e-12


def test_reference_head_needs_two_rows():
    from speakingstyle_amd import ops
    from speakingstyle_amd.ops import reference as ref

    x, w, b = torch.randn(1, 1, 128), torch.randn(18, 128, 7), torch.randn(18)
    with pytest.raises(ValueError):
        ref.istft_head(x, w, b, 16, 4)
    with pytest.raises(ValueError):
        ops.istft_head(x, w, b, 16, 4)


def test_ops_head_int16_is_clamp_and_convert():
    from speakingstyle_amd import ops

    torch.manual_seed(0)
    x, w, b = torch.randn(1, 9, 128), torch.randn(18, 128, 7) * 0.02, torch.randn(18) * 0.1
    y = ops.istft_head(x, w, b, 16, 4)
    yi = ops.istft_head(x, w, b, 16, 4, int16_scale=32768.0)
    assert yi.dtype == torch.int16 and torch.equal(yi, (y * 32768.0).clamp(-32768, 32767).to(torch.int16))


def test_generator_from_config_istft():
    from speakingstyle_amd.models.hifigan import Generator

    torch.manual_seed(0)
    g = Generator(_istft_config())
    assert g.hop == 256 and g.istft == (16, 4)
    assert tuple(g.conv_post.weight_v.shape) == (18, 128, 7) and len(g.ups) == 2
    y = g(torch.randn(2, 80, 5))
    assert y.shape == (2, 1, 1280)
    y.pow(2).mean().backward()
    for conv in (g.conv_post, g.conv_pre):
        gr = conv.weight_v.grad
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().sum()) > 0
    g.eval()
    mel = torch.randn(2, 80, 5)
    with torch.no_grad():
        before = g(mel)
        after = g.fold_weight_norm()(mel)
        cl = g.infer(mel.transpose(1, 2).contiguous())
    assert not hasattr(g.conv_post, "weight_v")
    assert (before - after).abs().max().item() <= 1e-5
    # the channel-last inference path is the same function
    assert cl.shape == (2, 1280) and (cl - after[:, 0]).abs().max().item() <= 1e-5


def test_rates_times_hop_must_equal_hop_size():
    from speakingstyle_amd.models.hifigan import Generator

    h = _istft_config()
    h["gen_istft_hop_size"] = 2
    with pytest.raises(ValueError, match="gen_istft_hop_size"):
        Generator(h)
    h = _istft_config()
    h["upsample_rates"], h["upsample_kernel_sizes"] = [8, 4], [16, 8]
    with pytest.raises(ValueError, match="upsample_rates"):
        Generator(h)
    h = _istft_config()
    del h["gen_istft_hop_size"]
    with pytest.raises(ValueError, match="gen_istft_hop_size"):
        Generator(h)


def test_shipped_hifigan_config_is_unchanged():
    from speakingstyle_amd.models.hifigan import Generator
    from speakingstyle_amd.utils.model import vocoder_config

    h = vocoder_config()
    assert "gen_istft_n_fft" not in h and "gen_istft_hop_size" not in h
    g = Generator(h)
    assert g.istft is None and g.hop == 256 and g.conv_post.out_channels == 1
    assert tuple(g.conv_post.weight_v.shape) == (1, 32, 7)
    keys = set(g.state_dict().keys())
    want = {"conv_pre.bias", "conv_pre.weight_g", "conv_pre.weight_v", "conv_post.bias", "conv_post.weight_g",
            "conv_post.weight_v"}
    want |= {f"ups.{i}.{n}" for i in range(4) for n in ("bias", "weight_g", "weight_v")}
    want |= {f"resblocks.{j}.convs{c}.{k}.{n}" for j in range(12) for c in (1, 2) for k in range(3)
             for n in ("bias", "weight_g", "weight_v")}
    assert keys == want
    # the iSTFTNet state dict has the same module names (fewer stages), other shapes
    gi = Generator(_istft_config())
    assert set(gi.state_dict().keys()) < keys
    assert g.receptive_radius() >= 10 and gi.receptive_radius() >= 10


def test_get_vocoder_istftnet(tmp_path):
    from speakingstyle_amd.utils.model import get_vocoder

    mc = {"vocoder": {"model": "iSTFTNet", "speaker": "LJSpeech"}}
    g = get_vocoder(mc, torch.device("cpu"), ckpt_dir=str(tmp_path))
    assert g.istft == (16, 4) and g.hop == 256 and g.conv_post.out_channels == 18 and not g.training
    with pytest.raises(FileNotFoundError, match="generator_istft_LJSpeech"):
        get_vocoder(mc, torch.device("cpu"), ckpt_dir=str(tmp_path), allow_random=False)
    with pytest.raises(ValueError, match="iSTFTNet"):
        get_vocoder({"vocoder": {"model": "WaveGlow", "speaker": "LJSpeech"}}, torch.device("cpu"))
    h = get_vocoder({"vocoder": {"model": "HiFi-GAN", "speaker": "LJSpeech"}}, torch.device("cpu"),
                    ckpt_dir=str(tmp_path))
    assert h.istft is None and h.conv_post.out_channels == 1


def test_training_cli_trains_the_istft_generator(tmp_path):
    h = _istft_config()
    h.update(upsample_initial_channel=32, resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]],
             segment_size=2048, batch_size=2, num_workers=0)
    cfg = tmp_path / "config_istft.json"
    cfg.write_text(json.dumps(dict(h)))
    ck = tmp_path / "ck"
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "hifigan_train.py", "--synthetic", "--cpu", "--training_steps", "2",
                        "--config", str(cfg), "--checkpoint_path", str(ck), "--checkpoint_interval", "1",
                        "--validation_interval", "1", "--summary_interval", "1", "--stdout_interval", "1",
                        "--num_workers", "0"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Steps : 1," in r.stdout
    assert (ck / "g_00000001").exists() and (ck / "do_00000001").exists()
    saved = json.loads((ck / "config.json").read_text())
    assert saved["gen_istft_n_fft"] == 16 and saved["gen_istft_hop_size"] == 4
    blob = torch.load(ck / "g_00000001", weights_only=True)
    assert tuple(blob["generator"]["conv_post.weight_v"].shape) == (18, 8, 7)


@pytest.mark.parametrize("lengths,kernels,dilations", [
    ([9, 2, 5], [3], [[1]]),  # receptive radius 6 frames: the 2-frame utterance runs at 8 of the 9 frames
    ([40, 12, 25, 7], [3, 5], [[1, 2], [1, 3]])])  # radius 10: three groups
def test_bucketed_infer_equals_each_utterance_alone(lengths, kernels, dilations):
    """``infer(..., lengths=)`` truncates each length group at max_len + receptive_radius(): the valid samples of
    every utterance equal that utterance's row vocoded alone at the full padded length."""
    from speakingstyle_amd.models.hifigan import Generator

    h = _istft_config()
    h.update(upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], upsample_initial_channel=32,
             resblock_kernel_sizes=kernels, resblock_dilation_sizes=dilations, num_mels=8, hop_size=32)
    torch.manual_seed(0)
    g = Generator(h).eval()
    with torch.no_grad():  # larger weights than the 0.01 init so far-away frames actually matter
        for p in g.parameters():
            p.mul_(4.0)
    hop = g.hop
    assert hop == 32
    B, T = len(lengths), max(lengths)
    mel = torch.randn(B, T, 8)
    groups = g.length_buckets(lengths, T, g.receptive_radius(), 3, 0)
    assert min(w for _, w in groups) < T  # some utterance does run truncated
    out = g.infer(mel, lengths=lengths, max_buckets=3, bucket_cost=0)
    assert out.shape == (B, T * hop)
    alone = [g.infer(mel[b:b + 1])[0] for b in range(B)]
    for b, L in enumerate(lengths):
        torch.testing.assert_close(out[b, : L * hop], alone[b][: L * hop], rtol=1e-5, atol=1e-6)
    # truncating at the valid length instead (no halo) does change valid samples: the radius is needed
    g.receptive_radius = lambda: 0
    cut = g.infer(mel, lengths=lengths, max_buckets=3, bucket_cost=0)
    err = max((cut[b, : L * hop] - alone[b][: L * hop]).abs().max().item() for b, L in enumerate(lengths))
    assert err > 1e-4
