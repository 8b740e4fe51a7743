"""The MSE weight observer (`weight_observer: mse`, fqss_wq_observe_mse / fqss_wq_error of include/fqss.h): a NumPy oracle with the
header's fp32 quantizer arithmetic and fp64 sums, the seeded channel cases, and the check bodies that tests/test_wq_mse_cpu.py runs on
the CPU backend and tests/test_gpu_wq_mse.py on the HIP kernels."""
import copy
import functools

import numpy as np
import torch

STEPS, DEN = 81, 100
GAP_MIN = 1e-7          # the inputs must separate the best candidate from the runner-up by more than this (relative)
ERR_RTOL = 1e-12        # fp64 sums of at most ~10^4 non-negative terms in different orders: n * 2^-53 < 1e-12
F = np.float32
STAGE = 8192            # floats of one channel the HIP kernel parks in LDS (csrc/fq.hip kMseStage); STAGE + 1 re-reads memory
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1536, STAGE, STAGE + 1)     # STAGE: the longest staged channel (full-size ConvTasNet's decoder)
BITS = (2, 3, 4, 8)
KINDS = ("gauss", "laplace", "uniform", "outlier", "zero")
TINY = dict(n_spks=2, kernel_size=16, stride=8, n_filters=32, bn_chan=16, hid_chan=32, n_blocks=2, n_repeats=1)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def grid(n_bits):
    return F((1 << n_bits) - 1), F(-(1 << (n_bits - 1))), F((1 << (n_bits - 1)) - 1)


def channel_view(w, axis):
    """[C, outer * inner] rows in the kernels' element order (outer major, inner minor)"""
    w = np.asarray(w, dtype=F)
    outer = int(np.prod(w.shape[:axis], dtype=np.int64))
    C = w.shape[axis]
    return np.ascontiguousarray(w.reshape(outer, C, -1).transpose(1, 0, 2).reshape(C, -1))


def delta_of(lo, hi, L):
    return (F(2.0) * np.maximum(np.abs(lo), np.abs(hi))) / L


def quant_error(x, lo, hi, n_bits):
    """sum ((double)w - (double)(delta * q))^2 of one channel x (fp32 [n]) on the grid of (lo, hi): k_wq_fwd's operations in fp32"""
    L, qlo, qhi = grid(n_bits)
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = delta_of(F(lo), F(hi), L)
        q = np.fmin(np.fmax(np.rint(x / delta), qlo), qhi)
        y = (delta * q).astype(F)
    d = x.astype(np.float64) - y.astype(np.float64)
    return float(np.sum(d * d))


def ratio(k):
    return F(DEN - k) / F(DEN)


def search_rows(rows, n_bits):
    """channels [C, n] -> one dict(lo, hi, k, qmin, qmax, e [STEPS], gap) per channel: the contract of fqss_wq_observe_mse, candidates
    scanned in order with a strict <; gap = (second best - best) / best over the candidates (inf for a skipped search, whose `e` holds
    e_0 alone)"""
    rows = np.ascontiguousarray(rows, dtype=F)
    L, qlo, qhi = grid(n_bits)
    lo, hi = rows.min(axis=1), rows.max(axis=1)
    x64 = rows.astype(np.float64)
    e = np.empty((STEPS, rows.shape[0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(STEPS):
            delta = delta_of((ratio(k) * lo).astype(F), (ratio(k) * hi).astype(F), L)[:, None]
            q = np.fmin(np.fmax(np.rint(rows / delta), qlo), qhi)
            d = x64 - (delta * q).astype(F).astype(np.float64)
            e[k] = np.sum(d * d, axis=1)
    out = []
    for c in range(rows.shape[0]):
        amax = max(abs(lo[c]), abs(hi[c]))
        if not (amax > 0 and np.isfinite(amax)):
            out.append(dict(lo=lo[c], hi=hi[c], k=0, qmin=lo[c], qmax=hi[c], e=e[:1, c].copy(), gap=np.inf))
            continue
        ec, k = e[:, c], 0
        for j in range(1, STEPS):
            if ec[j] < ec[k]:
                k = j
        rest = np.delete(ec, k)
        gap = (rest.min() - ec[k]) / ec[k] if ec[k] > 0 else np.inf
        out.append(dict(lo=lo[c], hi=hi[c], k=k, qmin=F(ratio(k) * lo[c]), qmax=F(ratio(k) * hi[c]), e=ec.copy(), gap=gap))
    return out


def search(x, n_bits):
    return search_rows(np.asarray(x, dtype=F)[None, :], n_bits)[0]


def search_all(w, axis, n_bits):
    return search_rows(channel_view(w, axis), n_bits)


def make_channel(kind, n, rng):
    if kind == "gauss":
        return (rng.standard_normal(n) * 0.1).astype(F)
    if kind == "laplace":
        return (rng.laplace(size=n) * 0.1).astype(F)
    if kind == "uniform":
        return rng.uniform(-0.1, 0.1, n).astype(F)
    if kind == "outlier":
        x = (rng.standard_normal(n) * 0.1).astype(F)
        x[rng.integers(n)] = F(5.0)          # 50 sigma
        return x
    assert kind == "zero"
    return np.zeros(n, dtype=F)


def make_weight(kind, layout, C, length, seed):
    """a weight whose every channel has `length` values: axis 0 -> [C, Ci, k]; axis 1 -> [Ci, C, k] (outer = Ci > 1, inner = k > 1 where
    the length factors).  Returns (w, axis)."""
    rng = np.random.default_rng(seed)
    rows = np.stack([make_channel(kind, length, rng) for _ in range(C)])
    a, b = next(((length // k, k) for k in (3, 2, 5, 7, 16) if length % k == 0 and length // k > 1), (length, 1))
    if layout == 0:
        return np.ascontiguousarray(rows.reshape(C, a, b)), 0
    return np.ascontiguousarray(rows.reshape(C, a, b).transpose(1, 0, 2)), 1


def cases():
    """(kind, layout, C, length): every layout x channel count x length on Gaussian channels with the big sizes kept to few channels,
    every content x layout at the lengths around one and several waves, plus the staged / re-read boundary"""
    out = []
    for layout in (0, 1):
        for C in (1, 3, 300):
            for n in LENGTHS:
                if C == 300 and n > 257:
                    continue
                out.append(("gauss", layout, C, n))
        out.append(("gauss", layout, 300, 1536) if layout == 0 else ("laplace", layout, 3, STAGE + 1))
        for kind in KINDS[1:]:
            for n in (1, 65, 257, 1536):
                out.append((kind, layout, 3, n))
    return out


def case_seed(layout, C, length, n_bits):
    return 20261 + 1000 * length + 10 * C + layout + 7 * n_bits


def rel_close(got, want, rtol=ERR_RTOL):
    return abs(got - want) <= rtol * abs(want)


def gaps_ok(ref, length):
    """the condition on the inputs: the argmin must not hang on summation order.  A one-value channel has one-term sums, the same bits in
    any order: there exact ties do occur (a negative value at 3 bits ties candidates 12 and 13) and the tie rule decides"""
    return length == 1 or all(len(r["e"]) == 1 or r["gap"] > GAP_MIN for r in ref)


@functools.lru_cache(maxsize=None)
def observe_case(kind, layout, C, length, n_bits):
    """(w, axis, oracle result) of one case, computed once and shared.  With 300 channels a draw now and then holds a channel whose two
    best candidates are closer than GAP_MIN (seen: 6e-8 at 2 bits); the oracle alone decides that, and the next seed is drawn."""
    for attempt in range(4):
        w_np, axis = make_weight(kind, layout, C, length, seed=case_seed(layout, C, length, n_bits) + 100003 * attempt)
        ref = search_all(w_np, axis, n_bits)
        if gaps_ok(ref, length):
            break
    assert gaps_ok(ref, length), (kind, layout, C, length, n_bits, min(r["gap"] for r in ref))
    w_np.setflags(write=False)
    return w_np, axis, ref


def check_observe_case(K, kind, layout, C, length, n_bits, device):
    """fqss_wq_observe_mse on one weight against the oracle; returns the chosen k's and the error ratios best / min-max"""
    w_np, axis, ref = observe_case(kind, layout, C, length, n_bits)
    w = torch.from_numpy(w_np.copy()).to(device)
    shape = [1] * w.dim()
    shape[axis] = C
    lo0, hi0 = torch.full(shape, -0.5, device=device), torch.full(shape, 0.5, device=device)
    K.wq_observe(w, axis, lo0, hi0)
    outs = []
    for _ in range(2):
        qmin, qmax = torch.full(shape, -0.5, device=device), torch.full(shape, 0.5, device=device)
        k, err = K.wq_observe_mse(w, axis, qmin, qmax, n_bits, want=True)
        outs.append((qmin.cpu().numpy().reshape(-1), qmax.cpu().numpy().reshape(-1), k.cpu().numpy(), err.cpu().numpy()))
    for a, b in zip(*outs):        # two runs, the same bits
        assert a.tobytes() == b.tobytes(), (kind, layout, C, length, n_bits)
    qmin, qmax, k, err = outs[0]
    lo0, hi0 = lo0.cpu().numpy().reshape(-1), hi0.cpu().numpy().reshape(-1)
    for c, r in enumerate(ref):
        tag = (kind, layout, C, length, n_bits, c)
        assert F(lo0[c]).tobytes() == F(r["lo"]).tobytes() and F(hi0[c]).tobytes() == F(r["hi"]).tobytes(), tag
        assert int(k[c]) == r["k"], (tag, int(k[c]), r["k"], r["gap"])
        assert F(qmin[c]).tobytes() == F(r["qmin"]).tobytes() and F(qmax[c]).tobytes() == F(r["qmax"]).tobytes(), tag
        if r["k"] == 0:            # candidate 0 is the min/max observer's pair, bit for bit
            assert F(qmin[c]).tobytes() == F(lo0[c]).tobytes() and F(qmax[c]).tobytes() == F(hi0[c]).tobytes(), tag
        assert rel_close(err[c, 0], r["e"][0]) and rel_close(err[c, 1], r["e"][r["k"]]), (tag, err[c], r["e"][0], r["e"][r["k"]])
        if kind == "zero":
            assert (qmin[c], qmax[c], int(k[c])) == (0.0, 0.0, 0) and err[c, 0] == 0.0, tag
    # the quiet form (what the quantizer module calls) writes the same ranges
    q2min, q2max = torch.full(shape, -0.5, device=device), torch.full(shape, 0.5, device=device)
    assert K.wq_observe_mse(w, axis, q2min, q2max, n_bits) is None
    assert q2min.cpu().numpy().tobytes() == qmin.tobytes() and q2max.cpu().numpy().tobytes() == qmax.tobytes()
    return [r["k"] for r in ref], [r["e"][r["k"]] / r["e"][0] if r["e"][0] > 0 else 1.0 for r in ref]


def check_error_case(K, kind, layout, C, length, n_bits, device):
    """fqss_wq_error on arbitrary (not observed) ranges against the oracle, two runs bit-equal"""
    seed = 77 + 1000 * length + 10 * C + layout + 7 * n_bits
    w_np, axis = make_weight(kind, layout, C, length, seed=seed)
    rng = np.random.default_rng(seed + 1)
    lo = (-rng.uniform(0.02, 0.4, C)).astype(F)
    hi = rng.uniform(0.02, 0.4, C).astype(F)
    shape = [1] * w_np.ndim
    shape[axis] = C
    w = torch.from_numpy(w_np).to(device)
    tlo, thi = torch.from_numpy(lo.reshape(shape)).to(device), torch.from_numpy(hi.reshape(shape)).to(device)
    e1, p1 = K.wq_error(w, axis, tlo, thi, n_bits)
    e2, p2 = K.wq_error(w, axis, tlo, thi, n_bits)
    assert torch.equal(e1, e2) and torch.equal(p1, p2)
    rows = channel_view(w_np, axis)
    for c in range(C):
        want_e = quant_error(rows[c], lo[c], hi[c], n_bits)
        want_p = float(np.sum(rows[c].astype(np.float64) ** 2))
        assert rel_close(float(e1[c]), want_e) and rel_close(float(p1[c]), want_p), (kind, layout, C, length, n_bits, c, float(e1[c]), want_e)


def check_tie_rule(K, device):
    """exactly tied candidates: the smallest k wins.  One-value channels have one-term sums, so their e_k carry no summation order: a
    negative value at 3 bits clips to code -4 under every candidate from k = 1 on, the reconstruction -r_k |x| 8/7 overshoots at
    r = 0.88 by what it undershoots at r = 0.87, and for a power of two the two errors are the same double.  The all-zero channel
    ties the whole list at 0 and keeps candidate 0."""
    x = np.array([[-0.25], [-2.0], [0.0], [0.5]], dtype=F).reshape(4, 1, 1)
    ref = search_all(x, 0, 3)
    tied = [c for c, r in enumerate(ref) if len(r["e"]) > 1 and np.sum(r["e"] == r["e"][r["k"]]) > 1]
    assert tied, [r["k"] for r in ref]               # (the construction does tie)
    for c in tied:
        assert ref[c]["k"] == int(np.flatnonzero(ref[c]["e"] == ref[c]["e"].min())[0])
    w = torch.from_numpy(x).to(device)
    qmin, qmax = torch.full((4, 1, 1), -0.5, device=device), torch.full((4, 1, 1), 0.5, device=device)
    k, err = K.wq_observe_mse(w, 0, qmin, qmax, 3, want=True)
    k, err, qmin, qmax = k.cpu().numpy(), err.cpu().numpy(), qmin.cpu().numpy().reshape(-1), qmax.cpu().numpy().reshape(-1)
    for c, r in enumerate(ref):
        assert int(k[c]) == r["k"], (c, int(k[c]), r["k"])
        assert err[c, 0] == r["e"][0] and err[c, 1] == r["e"][r["k"]], c       # one-term sums: exact
        assert F(qmin[c]).tobytes() == F(r["qmin"]).tobytes() and F(qmax[c]).tobytes() == F(r["qmax"]).tobytes(), c
    assert (int(k[2]), float(qmin[2]), float(qmax[2])) == (0, 0.0, 0.0)
    z = torch.zeros(2, 5, 3, device=device)
    qmin, qmax = torch.full((2, 1, 1), -0.5, device=device), torch.full((2, 1, 1), 0.5, device=device)
    k, err = K.wq_observe_mse(z, 0, qmin, qmax, 4, want=True)
    assert k.tolist() == [0, 0] and float(qmin.abs().max()) == 0.0 and float(qmax.abs().max()) == 0.0 and float(err.abs().max()) == 0.0


def check_bad_args(K, FqssError, pytest, device):
    w = torch.randn(4, 3, 2, device=device)
    lo, hi = -torch.ones(4, 1, 1, device=device), torch.ones(4, 1, 1, device=device)
    for n in (1, 9):
        with pytest.raises(FqssError, match="2..8"):
            K.wq_observe_mse(w, 0, lo, hi, n)
        with pytest.raises(FqssError, match="2..8"):
            K.wq_error(w, 0, lo, hi, n)
    assert float(lo.min()) == -1.0 and float(hi.max()) == 1.0      # a refused call writes nothing


# ------------------------------------------------------------------------------------------------ through the model
def qcfg(n_bits, **over):
    from fqss_amd.smoke import QCFG
    return dict(QCFG, weight_n_bits=n_bits, **over)


def normal_weights(model, seed=11):
    """bell-shaped conv / linear weights (PyTorch's default init is uniform, where clipping buys nothing)"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() >= 2:
                p.copy_(torch.randn(p.shape, generator=gen) * float(p.std()) if p.numel() > 1 else p)
    return model


def tiny_convtasnet(device, n_bits, observer="mse", seed=0):
    from fqss_amd.quantization.qat.models.convtasnetq import ConvTasNetQ
    from fqss_amd.quantization.qat.models.load_model import quantize_model
    torch.manual_seed(seed)
    model = normal_weights(ConvTasNetQ(**TINY))
    fmodel = copy.deepcopy(model)
    cfg = qcfg(n_bits) if observer is None else qcfg(n_bits, weight_observer=observer)
    return quantize_model(model, cfg).to(device).train(), fmodel.to(device).eval()


def weight_quantizers(model):
    from fqss_amd.quantization.qat import qat_quant as QQ
    return [m for m in model.modules() if isinstance(m, QQ.GradientWeightFakeQuantize)]


def check_ranges_after_first_forward(K, model, ref_keys, n_bits, expect_strict=True):
    """after one training forward of a `weight_observer: mse` model: every weight quantizer's ranges equal the oracle's for its weight,
    observer_mode is False everywhere, the key list is the min/max model's, and the error of the chosen ranges is <= that of min/max
    per channel (strictly lower over the model when its weights are bell-shaped).  Returns (model error, min/max error)."""
    from fqss_amd.quantization.qat.qat_utils import weight_quantizer_pairs
    assert list(model.state_dict().keys()) == list(ref_keys)
    wqs = weight_quantizers(model)
    assert wqs and all(not m.observer_mode and m.observer == "mse" and m.n_bits == n_bits for m in wqs)
    owners = weight_quantizer_pairs(model)
    assert len(owners) == len(wqs), (len(owners), len(wqs))
    tot, tot0 = 0.0, 0.0
    for wqm, w, pname in owners:
        wd = w.detach()
        rows = channel_view(wd.cpu().numpy(), wqm.axis)
        ref = search_rows(rows, n_bits)
        qmin, qmax = wqm.min_range.detach().cpu().numpy().reshape(-1), wqm.max_range.detach().cpu().numpy().reshape(-1)
        for c, r in enumerate(ref):
            assert rows.shape[1] == 1 or r["gap"] > GAP_MIN, (pname, c, r["gap"])          # the condition on the inputs (seeded weights)
            assert F(qmin[c]).tobytes() == F(r["qmin"]).tobytes() and F(qmax[c]).tobytes() == F(r["qmax"]).tobytes(), (pname, c, r["k"])
        lo0, hi0 = torch.empty_like(wqm.min_range.data), torch.empty_like(wqm.max_range.data)
        K.wq_observe(wd, wqm.axis, lo0, hi0)
        e, _ = K.wq_error(wd, wqm.axis, wqm.min_range.data, wqm.max_range.data, n_bits)
        e0, _ = K.wq_error(wd, wqm.axis, lo0, hi0, n_bits)
        assert bool((e <= e0).all()), pname
        tot, tot0 = tot + float(e.sum()), tot0 + float(e0.sum())
    assert tot <= tot0 and (tot < tot0 or not expect_strict), (tot, tot0)
    return tot, tot0


def oracle_report(model):
    """{parameter name: (SQNR dB, share of channels narrower than min/max)} from the oracle"""
    from fqss_amd.quantization.qat.qat_utils import weight_quantizer_pairs
    out = {}
    for wqm, w, pname in weight_quantizer_pairs(model):
        rows = channel_view(w.detach().cpu().numpy(), wqm.axis)
        qmin, qmax = wqm.min_range.detach().cpu().numpy().reshape(-1), wqm.max_range.detach().cpu().numpy().reshape(-1)
        err = sum(quant_error(rows[c], qmin[c], qmax[c], wqm.n_bits) for c in range(len(rows)))
        pw = float(np.sum(rows.astype(np.float64) ** 2))
        narrower = sum(bool((F(qmax[c]) - F(qmin[c])) < (F(rows[c].max()) - F(rows[c].min()))) for c in range(len(rows))) / len(rows)
        out[pname] = (10.0 * np.log10(pw / err), float(narrower))
    return out


def check_report(model, rows):
    """qat_utils.weight_quant_report against the oracle: one row per quantized weight, SQNR within 1e-9 dB"""
    from fqss_amd.quantization.qat.qat_utils import weight_quantizer_pairs
    want = oracle_report(model)
    owners = weight_quantizer_pairs(model)
    assert [r["name"] for r in rows] == [pname for _, _, pname in owners] and len(rows) == len(weight_quantizers(model))
    for r, (wqm, _, pname) in zip(rows, owners):
        assert set(r) == {"name", "n_bits", "channels", "sqnr_db", "narrower"}
        assert r["n_bits"] == wqm.n_bits and r["channels"] == wqm.min_range.numel(), r
        assert abs(r["sqnr_db"] - want[pname][0]) <= 1e-9 and r["narrower"] == want[pname][1], (r, want[pname])
    assert any(r["narrower"] > 0 for r in rows)


FAMILY_QCFG = dict(qat=True, gradient_based=True, weight_quant=True, act_quant=True, act_n_bits=8, in_quant=False, in_act_n_bits=8,
                   out_quant=True, out_act_n_bits=8, n_splitter=2, n_combiner=2, observer=True)


def family_pair(name, device, n_bits, observer="mse", seed=0):
    """tiny builds of the four model families as the family tests construct them (tests/test_gpu_dptnet.py, test_gpu_sepformer.py,
    test_gpu_htdemucs.py), with bell-shaped weights -> (quantized student in train mode, float teacher, step keywords)"""
    from fqss_amd.quantization.qat.models.load_model import quantize_model
    torch.manual_seed(seed)
    if name == "convtasnet":
        return tiny_convtasnet(device, n_bits, observer, seed) + (dict(kd_lambda=0.1, lr=1e-3, clip=5.0),)
    if name == "dptnet":
        from fqss_amd.quantization.qat.models.dptnetq import DPTNetQ
        model = DPTNetQ(n_spks=2, kernel_size=2, enc_dim=16, feature_dim=8, hidden_dim=12, layer=2, segment_size=10)
        kw = dict(kd_lambda=0.1, lr=4e-4, clip=5.0)
    elif name == "sepformer":
        from fqss_amd.quantization.qat.models.sepformerq import MaskGenerator, SepformerQ
        model = SepformerQ(n_spks=2, kernel_size=16, stride=8, n_filters=16, n_repeats=1, n_heads=4, chunk_size=10)
        model.masker = MaskGenerator(2, 16, n_repeats=1, n_heads=4, chunk_size=10, n_ffn=32)
        kw = dict(kd_lambda=0.1, lr=1.5e-4, clip=5.0)
    else:
        assert name == "htdemucs"
        from fqss_amd.quantization.qat.models.htdemucsq import HTDemucsQ
        model = HTDemucsQ(sources=["a", "b"], audio_channels=2, channels=8, nfft=2048, depth=4, bottom_channels=16, t_layers=3, t_heads=2)
        kw = dict(kd_lambda=0.1, lr=3e-4, clip=0.0, loss="l1_sdr")
    model = normal_weights(model)
    fmodel = copy.deepcopy(model)
    cfg = dict(FAMILY_QCFG, weight_n_bits=n_bits)
    if observer is not None:
        cfg["weight_observer"] = observer
    return quantize_model(model, cfg).to(device).train(), fmodel.to(device).eval(), kw


def check_five_steps(model, fmodel, x, tgt, step_kw):
    """five training steps: finite losses, finite range gradients on every weight quantizer, some of them non-zero"""
    from fqss_amd.runtime import KDTrainStep
    step = KDTrainStep(model, fmodel, **step_kw)
    nonzero = 0
    for _ in range(5):
        r = step(x, tgt)
        assert np.isfinite(r["loss"].item())
        for m in weight_quantizers(model):
            for p in (m.min_range, m.max_range):
                assert p.grad is not None and bool(torch.isfinite(p.grad).all())
                nonzero += int(float(p.grad.abs().max()) > 0.0)
    assert nonzero >= len(weight_quantizers(model))          # (of 10 per quantizer: most ranges do receive a gradient)
    return step
