"""LSTMQ_static (`model_cfg.quantization.lstm_quant: static`) without a GPU: the module's state_dict surface against the reference's
(tests/golden/lstmq_static.npz, tools/make_goldens_lstmq.py), the configuration key through load_model / DPTNetQ / qat_utils, and
loading a reference-style checkpoint."""
import numpy as np
import pytest
import torch
import torch.nn as nn

P = dict(gradient_based=True, weight_quant=True, act_quant=True, act_n_bits=8, weight_n_bits=8)
TINY = dict(n_spks=2, kernel_size=2, enc_dim=16, feature_dim=8, hidden_dim=12, layer=2, segment_size=10)


def _layer(H=8, **over):
    from fqss_amd.quantization.qat import qat_layers as QL
    return QL.LSTMQ_static(nn.LSTM(16, H, 1, bidirectional=True), **dict(P, **over))


def test_state_dict_surface_is_the_references(golden):
    from fqss_amd.quantization.qat import qat_layers as QL
    from fqss_amd.quantization.qat.qat_quant import GradientActivationFakeQuantize, _BypassQuantizer
    g = golden("lstmq_static")
    L = _layer()
    assert isinstance(L, QL.LSTMQ)
    sd = L.state_dict()
    assert list(sd) == list(g["keys"])
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == list(g["shapes"])
    steps = [n for n, m in L.named_children() if n.startswith("activation_fake_quantize_")]
    assert len(steps) == 24 and all(isinstance(getattr(L, n), GradientActivationFakeQuantize) for n in steps)
    off = _layer(act_quant=False)
    assert all(isinstance(getattr(off, n), _BypassQuantizer) for n in steps) and isinstance(off.activation_fake_quantize, _BypassQuantizer)
    assert not any("activation_fake_quantize" in k for k in off.state_dict())


def test_reference_style_state_dict_loads_strictly(golden):
    g = golden("lstmq_static")
    for case, H in (("q8", 8), ("q24", 24), ("cal", 8)):
        sd = {k[len(case) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(case + ".sd.")}
        L = _layer(H)
        L.load_state_dict(sd, strict=True)
        assert L.activation_fake_quantize_hh_r.min_range.item() == float(g[f"{case}.sd.activation_fake_quantize_hh_r.min_range"][0])
    assert L.activation_fake_quantize_mul2_r.min_range.item() == -0.5 and L.activation_fake_quantize_mul2_r.max_range.item() == 0.5


def test_lstm_quant_key_selects_the_class(golden):
    from fqss_amd.quantization.qat import qat_layers as QL
    from fqss_amd.quantization.qat.models.dptnetq import DPTNetQ, TransformerEncoderLayer
    from fqss_amd.quantization.qat.models.load_model import quantize_model
    from fqss_amd.smoke import QCFG
    m = quantize_model(DPTNetQ(**TINY), dict(QCFG, lstm_quant="static"))
    layers = [t for t in m.modules() if isinstance(t, TransformerEncoderLayer)]
    assert len(layers) == 4 and all(type(t.lstm) is QL.LSTMQ_static for t in layers)
    step_keys = [k for k in m.state_dict() if ".lstm.activation_fake_quantize_" in k]
    assert len(step_keys) == 4 * 24 * 2
    # absent (and the explicit default): today's model, key for key
    g = golden("dpt_tiny_step")
    for cfg in (dict(QCFG), dict(QCFG, lstm_quant="weights")):
        m = quantize_model(DPTNetQ(**TINY), cfg)
        assert all(type(t.lstm) is QL.LSTMQ for t in m.modules() if isinstance(t, TransformerEncoderLayer))
        assert list(m.state_dict().keys()) == list(g["sd_keys"])


def test_bad_lstm_quant_value_raises():
    from fqss_amd.quantization.qat import qat_utils
    from fqss_amd.quantization.qat.models.convtasnetq import ConvTasNetQ
    from fqss_amd.quantization.qat.models.dptnetq import DPTNetQ
    from fqss_amd.quantization.qat.models.load_model import quantize_model
    from fqss_amd.smoke import QCFG
    for bad in ("dynamic", "Static", True, 8):
        with pytest.raises(ValueError, match="weights.*static"):
            quantize_model(DPTNetQ(**TINY), dict(QCFG, lstm_quant=bad))
    with pytest.raises(ValueError, match="weights.*static"):
        DPTNetQ(**TINY).quantize_model(lstm_quant="dynamic")
    with pytest.raises(ValueError, match="weights.*static"):
        qat_utils.quant_lstm(nn.LSTM(16, 8, 1, bidirectional=True), dict(P, lstm_quant="full"))
    assert type(qat_utils.quant_lstm(nn.LSTM(16, 8, 1, bidirectional=True), dict(P))).__name__ == "LSTMQ"
    with pytest.raises(NotImplementedError, match="DPTNet"):
        quantize_model(ConvTasNetQ(n_spks=2), dict(QCFG, lstm_quant="static"))


def test_shipped_config_selects_static():
    import os
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "configs", "dptnet_2spks_8k_synthetic_lstmq.yaml")) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(root, "configs", "dptnet_2spks_8k_synthetic.yaml")) as f:
        base = yaml.safe_load(f)
    assert cfg["model_cfg"]["quantization"].pop("lstm_quant") == "static"
    cfg.pop("work_dir"), base.pop("work_dir")
    assert cfg == base


def test_fixture_holds_data_only(golden):
    g = golden("lstmq_static")
    assert all(g[k].dtype.kind in "fiU" for k in g.files)
    used = [k for k in g.files if k.startswith("q8.grad.activation_fake_quantize_")]
    assert len(used) == 46 and not any("mul2_r" in k for k in used) and all(float(np.abs(g[k]).max()) > 0 for k in used)
    n = dict(zip(g["cal.quantizers"], g["cal.n_iter"]))
    assert n["activation_fake_quantize_mul2_r"] == 0 and n["activation_fake_quantize_mul2"] == 50 and n["activation_fake_quantize"] == 1
