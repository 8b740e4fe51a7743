"""Step runtime: flat parameter arena, fused clip+Adam, and the KD training step.

MI355X-first choices:
  * ONE flat fp32 buffer each for parameters, gradients and the two Adam moments: kernels accumulate
    parameter gradients straight into the flat gradient buffer (no per-parameter AccumulateGrad
    kernels), the optimizer is two launches over the whole model, and data-parallel training
    all-reduces that one buffer over RCCL/xGMI.
  * nothing on the step reads device memory from the host (the reference syncs ~400x per forward,
    qat_quant.py:235-238), so the whole step can be captured in a hipGraph.
"""
import operator
import os

import torch

from . import _lib
from . import kernels as K
from . import ops
from . import ops_dp


class ParamArena:
    def __init__(self, params, align=64, accumulator=False):
        params = [p for p in params if p.requires_grad]
        assert params, "no trainable parameters"
        dev = params[0].device
        assert dev.type == ("cpu" if _lib.BACKEND == "cpu" else "cuda"), "ParamArena: parameters must live where the selected backend computes"
        offs, n = [], 0
        for p in params:
            offs.append(n)
            n += (p.numel() + align - 1) // align * align
        self.params, self.offsets, self.numel = params, offs, n
        self.flat_p = torch.zeros(n, device=dev)
        self.flat_g = torch.zeros(n, device=dev)
        self.exp_avg = torch.zeros(n, device=dev)
        self.exp_avg_sq = torch.zeros(n, device=dev)
        self.sumsq = torch.zeros(1, device=dev, dtype=torch.float64)
        self.step_t = torch.zeros(1, device=dev, dtype=torch.int32)
        self.gnorm = torch.zeros(1, device=dev)
        # gradient accumulation only (KDTrainStep(accumulate=N > 1)): the sum of a window's micro-batch gradients while the next
        # micro-batch rewrites flat_g.  Empty between windows, so it is not state
        self.acc = torch.zeros(n, device=dev) if accumulator else None
        # torch.optim.Adam counts steps per parameter, from the first step the parameter has a gradient
        self.t0 = torch.full((n,), 2 ** 31 - 1, device=dev, dtype=torch.int32)
        self._inactive = list(zip(params, offs))
        self._host_step = 0
        with torch.no_grad():
            for p, o in zip(params, offs):
                v = self.flat_p[o:o + p.numel()].view(p.shape)
                v.copy_(p.data)
                p.data = v
                p.grad = self.flat_g[o:o + p.numel()].view(p.shape)
                p._fqss_direct = True

    def zero_grad(self):
        self.flat_g.zero_()

    # ---- training-state checkpoint (fqss_amd/checkpoint.py) -----------------------------------
    NEVER = 2 ** 31 - 1         # t0 of an element that has not seen a gradient yet

    def layout(self):
        """what a stored arena must agree on to be loaded here: parameter names (set by the owning step; positions otherwise), offsets
        and sizes in the flat buffers"""
        names = getattr(self, "names", None) or [f"p{i}" for i in range(len(self.params))]
        return {"names": list(names), "offsets": [int(o) for o in self.offsets], "numel": [int(p.numel()) for p in self.params],
                "total": int(self.numel)}

    def state_dict(self):
        """host copies of the parameters, the two Adam moments and both Adam clocks (the device counter step_t, the per-element
        first-gradient step t0, the host's _host_step), with the layout they belong to.  The gradient buffer is rewritten by every
        step and is not state."""
        c = lambda t: t.detach().cpu().clone()
        return {"layout": self.layout(), "flat_p": c(self.flat_p), "exp_avg": c(self.exp_avg), "exp_avg_sq": c(self.exp_avg_sq),
                "step_t": c(self.step_t), "t0": c(self.t0), "host_step": int(self._host_step)}

    def load_state_dict(self, sd):
        """INTO the existing flat buffers: the views that p.data / p.grad hold (and every device table built on their addresses)
        stay valid.  Parameters are matched BY NAME: the order of the arena follows the gradient buckets (world size, `buckets`), so a
        file written under another order is copied slice by slice from its offsets to this arena's.  Refused: a file whose set of
        names or whose size of any parameter differs.  `_inactive` is rebuilt from t0: a parameter is inactive while its elements
        still sit at INT32_MAX."""
        mine, theirs = self.layout(), sd["layout"]
        here, there = dict(zip(mine["names"], mine["numel"])), dict(zip(theirs["names"], theirs["numel"]))
        if here != there:
            odd = [n for n in mine["names"] if n not in there] + [n for n in theirs["names"] if n not in here]
            sized = [f"{n}: {here[n]} here, {there[n]} in the file" for n in mine["names"] if n in there and here[n] != there[n]]
            raise ValueError(f"ParamArena.load_state_dict: the stored arena layout does not match this model ({len(here)} parameters here, "
                             f"{len(there)} in the file" + (f"; first differing name: {odd[0]!r}" if odd else "")
                             + (f"; first differing size: {sized[0]}" if sized else "") + ")")
        for k in ("flat_p", "exp_avg", "exp_avg_sq", "t0"):
            if sd[k].dtype != getattr(self, k).dtype or sd[k].numel() != theirs["total"]:
                raise ValueError(f"ParamArena.load_state_dict: {k} is {tuple(sd[k].shape)} {sd[k].dtype} in the file, expected "
                                 f"({theirs['total']},) {getattr(self, k).dtype}")
        with torch.no_grad():
            if mine == theirs:
                for k in ("flat_p", "exp_avg", "exp_avg_sq", "t0"):
                    getattr(self, k).copy_(sd[k])
            else:
                # another order: gather on the host into this arena's order (padding: no moments, no clock), one upload per buffer
                at = dict(zip(theirs["names"], theirs["offsets"]))
                for k in ("flat_p", "exp_avg", "exp_avg_sq", "t0"):
                    src = sd[k].cpu()
                    dst = torch.full((self.numel,), self.NEVER, dtype=src.dtype) if k == "t0" else torch.zeros(self.numel, dtype=src.dtype)
                    for n, o, m in zip(mine["names"], mine["offsets"], mine["numel"]):
                        dst[o:o + m] = src[at[n]:at[n] + m]
                    getattr(self, k).copy_(dst)
            self.step_t.copy_(sd["step_t"])
            self.flat_g.zero_()
        self._host_step = int(sd["host_step"])
        t0 = self.t0.cpu()
        self._inactive = [(p, o) for p, o in zip(self.params, self.offsets) if int(t0[o]) == self.NEVER]

    def _activate_touched(self):
        if self._inactive:
            still = []
            for p, o in self._inactive:
                if getattr(p, "_fqss_touched", False):
                    self.t0[o:o + p.numel()] = self._host_step
                else:
                    still.append((p, o))
            self._inactive = still
        self._host_step += 1

    def clip_adam_step(self, lr, max_norm=5.0, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8, activate=True):
        if activate:
            self._activate_touched()
        self.sumsq.zero_()
        K.sumsq(self.flat_g, self.sumsq)
        K.adam_clip(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.sumsq, self.step_t, self.gnorm,
                    max_norm, grad_scale, lr, betas[0], betas[1], eps, t0=self.t0)

    def decay_table(self, param_decay, weight_decay=0.0):
        """param_decay {parameter name: its own weight decay} over the scalar `weight_decay` -> the per-slot table of fqss_optim_clip
        (one fp32 value per 64 floats of the arena; slices start and end on slot boundaries), or None when no parameter departs
        from the scalar.  A name the arena does not hold raises."""
        if not param_decay:
            return None
        names = self.layout()["names"]
        unknown = sorted(set(param_decay) - set(names))
        if unknown:
            raise ValueError(f"param_decay names parameters the arena does not hold: {unknown[:3]}")
        for n, wd in param_decay.items():
            if not float(wd) >= 0.0:
                raise ValueError(f"param_decay[{n!r}] must be >= 0, got {wd!r}")
        if all(float(wd) == float(weight_decay) for wd in param_decay.values()):
            return None
        assert self.numel % 64 == 0 and all(o % 64 == 0 for o in self.offsets), "the decay table needs 64-float slots"
        table = torch.full((self.numel // 64,), float(weight_decay), dtype=torch.float32)
        for n, p, o in zip(names, self.params, self.offsets):
            if n in param_decay:
                table[o // 64:(o + p.numel() + 63) // 64] = float(param_decay[n])
        return table.to(self.flat_p.device)

    def clip_optim_step(self, lr, max_norm=5.0, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8, activate=True, kind="adam",
                        weight_decay=0.0, momentum=0.0, nesterov=False, wd_slot=None):
        """clip + update with any optimizer of the family.  The default configuration -- adam, no decay anywhere, no table -- IS
        clip_adam_step: the same two launches (fqss_sumsq, fqss_adam_clip), so the default run's graphs and bench.py's path do not
        change; everything else goes to fqss_optim_clip.  SGD keeps its momentum buffer in exp_avg."""
        if kind not in K.OPT_KINDS:
            raise ValueError(f"unknown optimizer {kind!r}: one of {sorted(K.OPT_KINDS)}")
        if kind == "adam" and float(weight_decay) == 0.0 and wd_slot is None:
            return self.clip_adam_step(lr, max_norm, grad_scale, betas, eps, activate)
        if activate:
            self._activate_touched()
        self.sumsq.zero_()
        K.sumsq(self.flat_g, self.sumsq)
        K.optim_clip(self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.sumsq, self.step_t, self.gnorm, max_norm,
                     grad_scale, lr, betas[0], betas[1], eps, t0=self.t0, kind=kind, weight_decay=weight_decay, wd_slot=wd_slot,
                     momentum=momentum, nesterov=nesterov)


TEACHER_STREAM = True    # False: the teacher forward on the step's own stream (tests and tools/stress_step.py patch it)


def _teacher_stream():
    return torch.cuda.Stream(priority=0)


class TeacherRunner:
    """Frozen float ConvTasNet teacher as a fused inference chain (csrc/teacher.hip): 3 kernels per TCN
    block, weights pre-split once into exact bf16 planes.  Falls back to the module forward for any other
    teacher structure."""

    def __init__(self, fmodel):
        import torch.nn as nn
        from .quantization.qat.models.convtasnetq import ConvBlock, ConvTasNetQ
        self.fmodel = fmodel
        self.ok = False
        m = fmodel
        try:
            ok = isinstance(m, ConvTasNetQ) and type(m.encoder) is nn.Conv1d and type(m.decoder) is nn.ConvTranspose1d
            mk = m.masker
            ok = ok and type(mk.bottleneck[0]) is nn.GroupNorm and type(mk.bottleneck[1]) is nn.Conv1d
            ok = ok and type(mk.mask_net[0]) is nn.PReLU and type(mk.mask_net[1]) is nn.Conv1d and type(mk.mask_net[2]) is nn.ReLU
            for blk in mk.TCN:
                sb = blk.shared_block
                ok = ok and isinstance(blk, ConvBlock) and [type(t) for t in sb] == [nn.Conv1d, nn.PReLU, nn.GroupNorm, nn.Conv1d,
                                                                                   nn.PReLU, nn.GroupNorm]
                ok = ok and type(blk.res_conv) is nn.Conv1d and type(blk.skip_conv) is nn.Conv1d and sb[3].kernel_size[0] <= 8
                ok = ok and sb[0].in_channels % 8 == 0 and sb[0].out_channels % 8 == 0
            ok = ok and m.n_splitter == 1 and m.n_combiner == 1 and m.encoder.bias is None and m.decoder.bias is None
            ok = ok and m.decoder.out_channels == 1 and m.encoder.in_channels == 1 and m.encoder.kernel_size[0] in (16, 32)
            self.ok = bool(ok)
        except AttributeError:
            self.ok = False
        self._planes = None

    def _prepare(self):
        mk = self.fmodel.masker
        P = lambda conv: K.split3_planes(conv.weight.detach().reshape(conv.out_channels, conv.in_channels))
        blocks = []
        for blk in mk.TCN:
            sb = blk.shared_block
            rs_w = torch.cat([blk.res_conv.weight.detach(), blk.skip_conv.weight.detach()], 0)
            rs_b = torch.cat([blk.res_conv.bias.detach(), blk.skip_conv.bias.detach()], 0).contiguous()
            blocks.append((P(sb[0]), K.split3_planes(rs_w.reshape(rs_w.shape[0], rs_w.shape[1])), rs_b))
        self._planes = dict(bn=P(mk.bottleneck[1]), mask=P(mk.mask_net[1]), blocks=blocks)

    @torch.no_grad()
    def __call__(self, x):
        if not self.ok or (x.shape[-1] - self.fmodel.encoder.kernel_size[0]) // self.fmodel.encoder.stride[0] + 1 > 12 * 1024:
            return self.fmodel(x)     # (the fused depthwise stage keeps a whole row of frames in LDS)
        if self._planes is None:
            self._prepare()
        m, mk, pl = self.fmodel, self.fmodel.masker, self._planes
        if x.dim() == 2:
            x = x.unsqueeze(1)
        B = x.shape[0]
        stride = m.encoder.stride[0]
        feats = K.frames_conv_fwd(x, m.encoder.weight, stride)                       # [B, F, M]
        nb = len(mk.TCN)
        st = K.tstat_buffer(1 + 2 * nb, B, x.device)                                 # GroupNorm (sum, sum^2) partials per sample
        K.tstats(feats, st[0])
        gn0, bn = mk.bottleneck[0], mk.bottleneck[1]
        h = K.tgemm(pl["bn"], feats, bn.bias, pro=1, pro_stats=st[0], pro_gamma=gn0.weight, pro_beta=gn0.bias, pro_eps=gn0.eps)
        acc = None
        nfeat = h.shape[1]
        for i, blk in enumerate(mk.TCN):
            sb = blk.shared_block
            p_c1, p_rs, b_rs = pl["blocks"][i]
            y1 = K.tgemm(p_c1, h, sb[0].bias, act=K.ACT_PRELU, slope=sb[1].weight, stats_out=st[1 + 2 * i])
            y3 = K.tdw(y1, st[1 + 2 * i], sb[2].weight, sb[2].bias, sb[2].eps, sb[3].weight, sb[3].bias, sb[4].weight,
                       st[2 + 2 * i], sb[3].dilation[0], sb[3].padding[0])
            h, acc = K.tgemm(p_rs, y3, b_rs, pro=1, pro_stats=st[2 + 2 * i], pro_gamma=sb[5].weight, pro_beta=sb[5].bias,
                             pro_eps=sb[5].eps, M1=nfeat, r1=h, r2=acc)
        mask = K.tgemm(pl["mask"], acc, mk.mask_net[1].bias, act=K.ACT_RELU, pro=2, pro_slope=mk.mask_net[0].weight)
        F_ = feats.shape[1]
        if K.ola_convtr_ok(m.decoder.weight, stride):
            # the masking product is formed inside the decoder kernel (no [B, S, F, M] intermediate): same values, same sums
            dec = K.ola_convtr_mul_fwd(mask.reshape(B, m.n_srcs, F_, -1), feats, m.decoder.weight, stride)
        else:
            masked = K.mul_bcast_fwd(mask.reshape(B, m.n_srcs, F_, -1), feats)
            dec = K.ola_convtr_fwd(masked.reshape(B * m.n_srcs, F_, -1), m.decoder.weight, stride)
        return dec.reshape(B, m.n_srcs, -1)


class _LinearPair:
    """concatenated weight codes / dL/dW_q view of two same-input pointwise layers (ops.LinearActQPair)"""
    __slots__ = ("wc", "gw", "Co1", "partner")


class QuantTables:
    """Device-side descriptor tables that let ONE launch each do, for the whole model: the weight
    fake-quant forward (+ int8 codes), its backward, and the range/slope gradient flush (csrc/multi.hip).
    Built once the observer phase is over and the parameters live in a ParamArena (stable addresses)."""

    def __init__(self, model, arena, segments=None):
        """segments: list of parameter-id sets (forward order) -> finish_backward(k) only handles the quantizers whose parameters lie
        in segment k (the gradient all-reduce of a segment needs its weight / range / slope gradients final)"""
        import torch.nn as nn
        from .quantization.qat.qat_layers import LayerQ
        from .quantization.qat.qat_quant import GradientActivationFakeQuantize, GradientWeightFakeQuantize
        dev = arena.flat_p.device
        # ---- activation quantizers: one gacc arena, flush table ---------------------------------
        aqs = [m for m in model.modules() if isinstance(m, GradientActivationFakeQuantize)]
        slope_of = {}
        for layer in model.modules():
            if isinstance(layer, LayerQ) and isinstance(getattr(layer, "nl", None), nn.PReLU):
                slope_of[id(layer.activation_fake_quantize)] = layer.nl.weight
        self.gacc = torch.zeros(len(aqs), K.GACC_DOUBLES, dtype=torch.float64, device=dev)
        rows = []
        for i, m in enumerate(aqs):
            m._buffers["_gacc"] = self.gacc[i]
            m._fqss_deferred = True
            sl = slope_of.get(id(m))
            rows.append([self.gacc[i].data_ptr(), m.min_range.grad.data_ptr(), m.max_range.grad.data_ptr(),
                         sl.grad.data_ptr() if sl is not None else 0])
        self.flush_table = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.aqs = aqs
        # ---- weight quantizers --------------------------------------------------------------------
        from .quantization.qat.qat_layers import LSTMQ, MultiheadAttentionQ

        def fits(wqm, w):
            return isinstance(wqm, GradientWeightFakeQuantize) and isinstance(w, torch.nn.Parameter) and tuple(wqm.min_range.shape) == tuple(
                1 if d != wqm.axis else w.shape[d] for d in range(w.dim()))

        owners = []
        for layer in model.modules():
            wqm = getattr(layer, "weight_fake_quantize", None)
            if isinstance(wqm, GradientWeightFakeQuantize):
                # convolutions (channel-first and frame path) and the row-major linears of the dual-path / transformer layers
                for cand in ("conv1d", "convTr1d", "residual_encoder", "linear", "conv2d"):
                    conv = getattr(layer, cand, None)
                    if conv is not None and fits(wqm, getattr(conv, "weight", None)):
                        owners.append((wqm, conv.weight))
                        break
            if isinstance(layer, MultiheadAttentionQ):
                for wqm, w in ((layer.weight_fake_quantize_in, layer.mha.in_proj_weight), (layer.weight_fake_quantize_out, layer.mha.out_proj.weight)):
                    if fits(wqm, w):
                        owners.append((wqm, w))
            if isinstance(layer, LSTMQ):
                for name, wqm in layer.weight_quantizers_dict.items():
                    if fits(wqm, getattr(layer.lstm, name, None)):
                        owners.append((wqm, getattr(layer.lstm, name)))
        # layers declared as same-input pairs by their parent (`fqss_linear_pairs`) get adjacent storage: one
        # concatenated code image [Co1+Co2][Ci] (+ transposed, scales, row sums) and one dL/dW_q block, so that the
        # paired q-GEMMs (ops.LinearActQPair) see them as a single weight
        partner = {}
        for mod in model.modules():
            for n1, n2 in getattr(mod, "fqss_linear_pairs", ()):
                l1, l2 = getattr(mod, n1, None), getattr(mod, n2, None)
                w1 = getattr(getattr(l1, "conv1d", None), "weight", None)
                w2 = getattr(getattr(l2, "conv1d", None), "weight", None)
                own = {id(w) for _, w in owners}
                if w1 is None or w2 is None or id(w1) not in own or id(w2) not in own:
                    continue
                ok = w1.dim() == 3 and w1.shape[2] == 1 and w2.shape[1:] == w1.shape[1:] and K.q_eligible(w1.shape[1], w1.shape[0]) \
                    and K.q_eligible(w2.shape[1], w2.shape[0]) and (w1.numel() % 64 == 0) \
                    and (l1.conv1d.bias is None) == (l2.conv1d.bias is None)
                if ok:
                    partner[id(w1)] = w2
        second = {id(w2) for w2 in partner.values()}
        by_id = {id(w): (wqm, w) for wqm, w in owners}
        ordered = []
        for wqm, w in owners:
            if id(w) in second:
                continue
            ordered.append((wqm, w))
            if id(w) in partner:
                ordered.append(by_id[id(partner[id(w)])])
        owners = ordered
        n_gwq = sum((w.numel() + 63) // 64 * 64 for _, w in owners)
        self.gwq = torch.zeros(n_gwq, device=dev)                       # dL/dW_q arena (zeroed once per step)
        self.wq_store = torch.empty(n_gwq, device=dev)
        rows, off, blk = [], 0, 0
        self.weights = []
        self.pairs = []
        pending = None      # (pair codes, first wq, Co1) while the second member of a pair is being laid out
        for wqm, w in owners:
            shape, axis = tuple(w.shape), wqm.axis
            outer = 1
            for d in shape[:axis]:
                outer *= d
            inner = 1
            for d in shape[axis + 1:]:
                inner *= d
            C = shape[axis]
            wq = self.wq_store[off:off + w.numel()].view(shape)
            gwq = self.gwq[off:off + w.numel()].view(shape)
            pw = axis == 0 and w.dim() == 3 and shape[2] == 1 and K.q_eligible(shape[1], shape[0])
            # row-major linear weight [Co, Ci]: the same code image serves the int8 row GEMM (csrc/qrow.hip)
            pw = pw or (axis == 0 and w.dim() == 2 and ops_dp.QROW and K.qrow_eligible(shape[1]))
            # convolution weights [Co, Ci, k] / [Co, Ci, kh, kw] of the frame path (HTDemucs): the same code image over Ci * k "channels"
            # serves the DATA gradient alone (ops.LinearActQ: W_q^T gz on k_qgemm<1>); the forward reads float inputs
            fr = (not pw) and axis == 0 and w.dim() in (3, 4) and shape[0] % 16 == 0 and shape[0] <= 1024
            wc = None
            ldT = C
            if pw and id(w) in partner:
                # first of a pair: allocate the concatenated images, this layer's are views of rows / columns [0, Co1)
                w2 = partner[id(w)]
                Co1, Co2, Ci = shape[0], w2.shape[0], shape[1]
                pc = K.WCodes()
                pc.Co, pc.Ci = Co1 + Co2, Ci
                pc.idx = torch.empty(Co1 + Co2, Ci, device=dev, dtype=torch.int8)
                pc.idxT = torch.empty(Ci, Co1 + Co2, device=dev, dtype=torch.int8)
                pc.dw = torch.empty(Co1 + Co2, device=dev)
                pc.rw = torch.empty(Co1 + Co2, device=dev)
                pair = _LinearPair()
                pair.wc, pair.Co1 = pc, Co1
                pair.gw = self.gwq[off:off + w.numel() + w2.numel()].view(Co1 + Co2, Ci)
                pending = (pair, wq, 0)
            if pw and pending is not None:
                pair, wq_first, _ = pending
                pc = pair.wc
                r0 = 0 if wq_first is wq else pair.Co1
                wc = K.WCodes()
                wc.Co, wc.Ci = shape[0], shape[1]
                wc.idx = pc.idx[r0:r0 + shape[0]]
                wc.idxT = None                         # column block of pc.idxT (row stride Co1+Co2): paired kernels only
                wc.dw, wc.rw = pc.dw[r0:r0 + shape[0]], pc.rw[r0:r0 + shape[0]]
                ldT = pc.Co
                idxT_ptr = pc.idxT.data_ptr() + r0
                if wq_first is not wq:
                    pair.partner = wq
                    wq_first._fqss_pair = pair
                    self.pairs.append(pair)
                    pending = None
            elif pw or fr:
                wc = K.WCodes()
                wc.Co, wc.Ci = shape[0], (inner if fr else shape[1])
                wc.idx = torch.empty(wc.Co, wc.Ci, device=dev, dtype=torch.int8)
                wc.idxT = torch.empty(wc.Ci, wc.Co, device=dev, dtype=torch.int8)
                wc.dw = torch.empty(shape[0], device=dev)
                wc.rw = torch.empty(shape[0], device=dev)
                idxT_ptr = wc.idxT.data_ptr()
            coded = pw or fr
            rows.append([w.data_ptr(), wq.data_ptr(), wc.idx.data_ptr() if coded else 0, idxT_ptr if coded else 0,
                         wc.dw.data_ptr() if coded else 0, wc.rw.data_ptr() if coded else 0, wqm.min_range.data_ptr(),
                         wqm.max_range.data_ptr(), gwq.data_ptr(), w.grad.data_ptr(), wqm.min_range.grad.data_ptr(),
                         wqm.max_range.grad.data_ptr(), outer, C, inner, blk, ldT, int(wqm.n_bits)])
            wq._fqss_gwq = gwq
            if pw:
                wq._fqss_wcodes = wc
            elif fr:
                wq._fqss_wcodes_dgrad = wc
            w._fqss_wq = wq
            self.weights.append((wqm, w, wq, wc))
            off += (w.numel() + 63) // 64 * 64
            blk += C
        assert pending is None
        K.wq_table_check(rows)      # the launches cannot read the device table: widths (word 17) and extents are checked here
        self.wq_table = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.total_channels = blk
        # grouped, atomics-free weight gradients of the quantized 1x1 convolutions (csrc/qgemm.hip k_qwgrad_group); FQSS_GROUP_WGRAD=0:
        # one k_qwgrad2 launch per layer where autograd reaches it (rounds 2-4)
        self.det = None     # kernels.DetMode of the owning step (FQSS_DETERMINISTIC=1)
        grouped = os.environ.get("FQSS_GROUP_WGRAD", "1") != "0"
        self.wgrad_queue = K.WgradQueue() if grouped else None
        # ... and of the row-major linears of the dual-path / transformer models (csrc/gemm_x3.hip k_gemm_x3_wq_multi)
        self.row_wgrad_queue = K.RowWgradQueue() if grouped else None
        # bias gradients of the res convs whose output-quantizer backward ran in a dgrad epilogue (ops.FUSE_ADD_DGRAD): per layer a
        # workspace of per-workgroup row sums, reduced for all layers of a backward segment in ONE launch of finish_backward
        self._bias_ws, self._bias_jobs = {}, []
        # ---- per-segment views of the two finish tables (descriptor 15 = first block is renumbered per table) -----------------
        self.seg_tables = None
        if segments is not None and len(segments) > 1:
            self.seg_tables = []
            flush_rows = self.flush_table.tolist()
            for ids in segments:
                wrows, b0, members = [], 0, []
                for r, (wqm, w, _, _) in zip(rows, self.weights):
                    if id(w) in ids:
                        r = list(r)
                        r[15] = b0
                        b0 += r[13]
                        wrows.append(r)
                        members.append((wqm, w))
                frows = [r for r, m in zip(flush_rows, aqs) if id(m.min_range) in ids]
                self.seg_tables.append((torch.tensor(wrows, dtype=torch.int64, device=dev).reshape(-1, len(rows[0])), b0,
                                        torch.tensor(frows, dtype=torch.int64, device=dev).reshape(-1, 4), members))
            assert sum(t[0].shape[0] for t in self.seg_tables) == len(rows), "a weight quantizer belongs to no backward segment"
            assert sum(t[2].shape[0] for t in self.seg_tables) == len(flush_rows), "an activation quantizer belongs to no backward segment"

    def weights_forward(self):
        K.wq_multi_fwd(self.wq_table, self.total_channels)
        if self.wgrad_queue is not None:
            self.wgrad_queue.jobs = []        # (a backward that never reached finish_backward leaves nothing behind)
        if self.row_wgrad_queue is not None:
            self.row_wgrad_queue.jobs = []
        self._bias_jobs = []

    def bias_ws(self, gbias, B, C, M):
        """the workspace that fqss_qpw_bwd_x_addq fills for the layer whose bias gradient is `gbias`; queued for finish_backward"""
        nwg = K._lib.query("fqss_qpw_bwd_x_addq_wgs", B, M)
        key = (gbias.data_ptr(), nwg, C)
        ws = self._bias_ws.get(key)
        if ws is None:
            ws = self._bias_ws[key] = torch.empty(nwg * C, dtype=torch.float32, device=gbias.device)
        self._bias_jobs.append((ws, gbias, nwg, C))
        return ws

    def finish_backward(self, seg=None):
        """after autograd (of backward segment `seg`, or of the whole network): weight STE/range gradients from the dL/dW_q arena,
        then the range/slope flushes"""
        if self.wgrad_queue is not None:
            # the weight gradients of this segment's quantized 1x1 convolutions, queued by their autograd nodes (ops.LinearActQ /
            # LinearActQPair): ONE grouped launch per <= 25 layers, before the weight STE below reads the dL/dW_q arena
            self.wgrad_queue.flush()
        if self.row_wgrad_queue is not None:
            self.row_wgrad_queue.flush()
        if self._bias_jobs:
            K.bias_ws_reduce(self._bias_jobs)
            self._bias_jobs = []
        if self.det is not None:
            self.det.finish(1)      # FQSS_DETERMINISTIC=1: the depthwise / frame-path weight gradients' integer sums -> the dL/dW_q arena
        if seg is None or self.seg_tables is None:
            K.wq_multi_bwd(self.wq_table, self.total_channels)
            K.gacc_flush_multi(self.flush_table)
            members = [(wqm, w) for wqm, w, _, _ in self.weights]
        else:
            wt, nch, ft, members = self.seg_tables[seg]
            if wt.shape[0]:
                K.wq_multi_bwd(wt, nch)
            if ft.shape[0]:
                K.gacc_flush_multi(ft)
        for wqm, w in members:
            w._fqss_touched = wqm.min_range._fqss_touched = wqm.max_range._fqss_touched = True


class KDTrainStep:
    """one QAT step = student fwd + teacher fwd + KD loss + bwd (+ grad all-reduce) + clip + Adam
    (reference: System.training_step / common_step, mysystem.py:124-157; Adam + clip 5.0,
    asteroid_librimix_trainer.py:94,132).

    `capture()` records the step into two hipGraphs (fwd+loss+bwd | clip+Adam) once the model has
    left the observer phase; the step has no host sync, so replay needs no Python at all.  At N>1 the
    RCCL all-reduce of the flat gradient buffer runs between the two graphs."""

    def __init__(self, model, fmodel, kd_lambda=0.1, lr=1e-3, clip=5.0, comm=None, loss="sisdr_pit", source_weights=None,
                 batched_quantizers=True, fast=True, coded=True, buckets=None, sync_observer_ranges=True,
                 betas=(0.9, 0.999), loss_threshold=None, teacher_ahead=False, accumulate=1, optimizer="adam", weight_decay=0.0,
                 momentum=0.0, nesterov=False, param_decay=None, ema_decays=(), ema_epoch_decays=()):
        """loss: "sisdr_pit" = the asteroid KD loss (mysystem.py:124-151); "sisdr_pit_per_sample" = the speechbrain env's form of it
        (speechbrain_librimix_trainer.py:99-115, 141-149: log per sample, mean over the samples whose loss exceeds `loss_threshold`;
        per-GPU batch 1 or 2, see fqss_kd_loss_per_sample); "l1_sdr" = the htdemucs solver's
        (solver.py:333-366: L1 task + SDR-weighted L1 distillation, per-source weights).  clip <= 0: no clipping (htdemucs.yaml:84).
        batched_quantizers=False keeps every quantizer on its own launches (no QuantTables / codes-only dataflow);
        fast=False: quantizing layers also write their fp32 outputs (no carriers); coded=False: no layer output carries codes,
        every layer runs its un-fused fp32 kernels (the reference dataflow the tests pin the fused step against).
        buckets (world > 1, models with `fqss_segments`): the backward runs as that many separately launched segments and the
        gradient all-reduce of a finished segment overlaps the next segment's backward (default 4; 1 = one all-reduce after the
        whole backward).  sync_observer_ranges (world > 1): average the activation ranges over the ranks once, when the 50-call
        observer phase ends -- a documented deviation: the reference's DDP never re-synchronises the
        observer's .data writes (qat_quant.py:230-232), so its replicas quantize on different grids from then on.
        teacher_ahead: the frozen teacher's forward of the NEXT batch (`step(x, tgt, x_next=...)`) runs on the teacher stream beside
        this whole step -- forward AND backward -- instead of beside the student's forward only: it depends on nothing the step
        changes (mysystem.py:132-133 runs it under no_grad on the raw mixture), so a loader that knows the next batch can hide it
        behind the student's VALU / HBM-bound kernels.  Still one teacher forward per step; the step that finds no look-ahead
        result for its mixture (the first one, or a caller that did not announce it) runs the teacher beside its own forward as
        before.  Same values either way (tests/test_gpu_kdstep_path.py).
        accumulate = N: one optimizer update per window of N consecutive micro-batches (pl.Trainer(accumulate_grad_batches=N),
        speechbrain's grad_accumulation_factor): the update takes the SUM of the window's micro-batch gradients at grad_scale
        1 / (world * N) -- the data-parallel contract in time instead of space.  Each call runs one micro-batch; the N-th also
        exchanges and updates (`pending`: micro-batches of the open window).  micro_batch() / commit(keep) is the same in two
        halves for trainers that may drop a micro-batch, flush() ends a window early (end of an epoch).  1: the step as it always
        was -- no accumulator, the same launches, the one-graph replay.
        optimizer: "adam" | "adamw" | "sgd" with weight_decay, momentum / nesterov (sgd) -- torch.optim.Adam(weight_decay=) /
        AdamW / SGD(momentum, nesterov) on the clip and the per-parameter clocks of the fused update (fqss.h: fqss_optim_clip).
        param_decay {parameter name: decay}: parameters with a decay of their own (the reference's make_optim_group).  adam with no
        decay anywhere is the step as it always was: fqss_adam_clip, the same launches.
        ema_decays / ema_epoch_decays: exponential moving averages of the model (demucs' ModelEMA, unbias=True), one flat copy of
        the arena per decay.  The batch-level copies (ema_decays, numbered first) are updated by every optimizer update, inside the
        captured optimize graph; the epoch-level ones by ema_epoch_update().  ema_state(k) / ema_swap(k) read and borrow copy k."""
        if optimizer not in K.OPT_KINDS:
            raise ValueError(f"unknown optimizer {optimizer!r}: one of {sorted(K.OPT_KINDS)}")
        if not float(weight_decay) >= 0.0:
            raise ValueError(f"weight_decay must be >= 0, got {weight_decay!r}")
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError(f"momentum must lie in [0, 1), got {momentum!r}")
        if nesterov and not float(momentum) > 0.0:
            raise ValueError("nesterov needs a momentum > 0")
        if optimizer != "sgd" and (float(momentum) != 0.0 or nesterov):
            raise ValueError(f"momentum / nesterov belong to sgd; {optimizer}'s first-moment decay is betas[0]")
        self.optim = {"kind": optimizer, "weight_decay": float(weight_decay), "momentum": float(momentum), "nesterov": bool(nesterov),
                      "param_decay": {str(n): float(w) for n, w in (param_decay or {}).items()}}
        self.ema_kinds = ["batch"] * len(tuple(ema_decays)) + ["epoch"] * len(tuple(ema_epoch_decays))
        self.ema_decays = [float(d) for d in tuple(ema_decays) + tuple(ema_epoch_decays)]
        if any(not 0.0 <= d < 1.0 for d in self.ema_decays):
            raise ValueError(f"EMA decays must lie in [0, 1), got {self.ema_decays}")
        try:
            accumulate = operator.index(accumulate)
        except TypeError:
            raise ValueError(f"accumulate must be an integer >= 1, got {accumulate!r}") from None
        if accumulate < 1:
            raise ValueError(f"accumulate must be an integer >= 1, got {accumulate!r}")
        self.accumulate = accumulate
        self._pos = 0               # micro-batches committed in the open window (kept or dropped)
        self._kept = 0              # ... of which the accumulator holds this many
        self._open = False          # a micro-batch has run and waits for its commit()
        self._win_eager = False     # a micro-batch of the open window ran eagerly: its update activates parameters eagerly too
        self.model, self.fmodel = model, fmodel
        self.cpu = _lib.BACKEND == "cpu"
        if self.cpu:
            # cfg 1 (`--use_cpu`): the CPU backend serves the un-fused per-layer entry points only -- no codes-only dataflow, no batched
            # tables, no streams / graphs, the teacher as the plain module forward
            batched_quantizers = fast = coded = teacher_ahead = False
        self.teacher_ahead = bool(teacher_ahead)
        self.grad_at = None         # l1_sdr only, tests: evaluate dloss/dest at this output instead of the step's own (a parity gate against
                                    # reference gradients must not inherit the sign noise of |est - target| ~ 0 samples)
        self._ahead = None          # (mixture tensor, its version, teacher output) announced by the previous step
        self._tgraph = None         # captured teacher forward (teacher_ahead + hipGraph replay)
        self.loss_kind, self.source_weights, self.batched_quantizers = loss, source_weights, batched_quantizers
        if loss not in ("sisdr_pit", "sisdr_pit_per_sample", "l1_sdr"):
            raise ValueError(f"unknown loss {loss!r}")
        self.loss_threshold = loss_threshold       # per-sample objective only: samples at or below it leave the batch mean
        self.fast, self.coded = bool(fast and coded), bool(coded)
        self._graphs = None
        self.kd_lambda, self.lr, self.clip, self.betas = kd_lambda, lr, clip, tuple(betas)
        self.comm = comm
        # ---- backward segments = gradient buckets (world > 1 only: a single rank has nothing to overlap) -------------------
        self.segments = None        # [(arena lo, arena hi)] per segment in FORWARD order
        self._seg_ids = None
        self._sync_ranges = bool(sync_observer_ranges)
        self._ranges_synced = not (sync_observer_ranges and self._exchange())
        params = list(model.parameters())
        # FQSS_FORCE_BUCKETS=1 with a forced one-rank communicator (FQSS_FORCE_DIST=1): the bucketed schedule of world > 1 at world 1
        force_b = os.environ.get("FQSS_FORCE_BUCKETS", "0") == "1" and self._exchange()
        nb = (4 if buckets is None else int(buckets)) if (self._world() > 1 or force_b) else (int(buckets) if buckets else 1)
        if nb > 1 and hasattr(model, "fqss_segments"):
            segs = model.fqss_segments(nb)
            if len(segs) > 1:
                seen, ordered, self._seg_ids = set(), [], []
                for mods in segs:
                    ids = set()
                    for m in mods:
                        for p in m.parameters():
                            if id(p) not in seen:
                                seen.add(id(p))
                                ordered.append(p)
                            ids.add(id(p))
                    self._seg_ids.append(ids)
                rest = [p for p in params if id(p) not in seen]       # anything the model did not assign: with the first segment
                self._seg_ids[0] |= {id(p) for p in rest}
                params = rest + ordered
        self.arena = ParamArena(params, accumulator=accumulate > 1)
        name_of = {id(p): n for n, p in model.named_parameters()}
        self.arena.names = [name_of[id(p)] for p in self.arena.params]       # the layout a stored arena is checked against
        self._wd_slot = self.arena.decay_table(self.optim["param_decay"], self.optim["weight_decay"])
        # EMA copies: the arena's layout once more per decay, the count of the unbiased form beside them on the device, and the few
        # float32 state_dict entries the arena does not hold (buffers, frozen parameters).  A copy starts as the model (ModelEMA)
        self.ema = [self.arena.flat_p.clone() for _ in self.ema_decays]
        self.ema_count = torch.zeros(len(self.ema_decays), dtype=torch.float64, device=self.arena.flat_p.device)
        held = {id(p) for p in self.arena.params}
        self._ema_outside = [(n, t) for n, t in model.state_dict(keep_vars=True).items()
                             if t.dtype == torch.float32 and id(t) not in held] if self.ema_decays else []
        self.ema_extra = [{n: t.detach().clone() for n, t in self._ema_outside} for _ in self.ema_decays]
        # FQSS_DETERMINISTIC=1: bit-reproducible gradients (kernels.DetMode; no effect on the values beyond fp32 summation order)
        self.det = None
        if os.environ.get("FQSS_DETERMINISTIC", "0") == "1" and not self.cpu:
            self.det = K.DetMode()
            self.det.attach(0, self.arena.flat_g)
        if self._seg_ids is not None:
            off = {id(p): (o, o + (p.numel() + 63) // 64 * 64) for p, o in zip(self.arena.params, self.arena.offsets)}
            self.segments = []
            for ids in self._seg_ids:
                spans = [off[i] for i in ids if i in off]
                self.segments.append((min(a for a, _ in spans), max(b for _, b in spans)))
            assert all(self.segments[k][1] == self.segments[k + 1][0] for k in range(len(self.segments) - 1)), self.segments
        self._cstream = None
        self.comm_events = None     # bench.py: (end of the last backward segment, all exchanges joined) as timing events of a replay
        for p in fmodel.parameters():
            p.requires_grad_(False)
        self.teacher = TeacherRunner(fmodel)     # fused inference chain for the frozen float teacher
        if self.cpu:
            self.teacher.ok = False
        self._tstream = None
        self.last = None
        self.tables = None          # QuantTables once the quantizing phase is reached
        self._eager_q = 0           # eager steps run in the quantizing phase (see maybe_capture)
        self.use_graph = not self.cpu
        self._sx = self._st = None

    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        """the learning rate is an argument of the captured clip+Adam launch: a scheduler step drops the graphs (the trainers
        re-capture lazily, see maybe_capture)"""
        if getattr(self, "_lr", None) != value:
            self._graphs = None
        self._lr = value

    # ---- training-state checkpoint (fqss_amd/checkpoint.py; DESIGN.md "Resuming a run") ---------------------------------------
    def _quantizers(self):
        """(module path, module) of the activation and of the weight quantizers, in module order"""
        from .quantization.qat.qat_quant import GradientActivationFakeQuantize, GradientWeightFakeQuantize
        named = list(self.model.named_modules())
        return ([(n, m) for n, m in named if isinstance(m, GradientActivationFakeQuantize)],
                [(n, m) for n, m in named if isinstance(m, GradientWeightFakeQuantize)])

    def _ranks_differ(self):
        """world > 1: the ranks hold different activation ranges -- inside the observer phase until _maybe_sync_ranges has averaged
        them, and for good where that synchronisation was declined (sync_observer_ranges=False)"""
        return self._world() > 1 and (not self._sync_ranges or not self._ranges_synced)

    def _optim_block(self):
        """the checkpoint's `optim` entry: None for the default configuration (adam, no decay anywhere), whose files keep the keys they
        always had"""
        o = self.optim
        if o["kind"] == "adam" and o["weight_decay"] == 0.0 and self._wd_slot is None:
            return None
        return {"kind": o["kind"], "weight_decay": o["weight_decay"], "momentum": o["momentum"], "nesterov": o["nesterov"],
                "param_decay": dict(o["param_decay"]) if self._wd_slot is not None else {}}

    def _check_stored_optim(self, sd):
        """the moments of one optimizer mean nothing to another (SGD's buffer lives where Adam's first moment does), and an EMA copy
        belongs to its decay: a file written under another kind or another EMA list is refused, naming both"""
        default = {"kind": "adam", "weight_decay": 0.0, "momentum": 0.0, "nesterov": False, "param_decay": {}}
        mine, theirs = self._optim_block() or default, sd.get("optim") or default
        for key in ("kind", "momentum", "nesterov"):
            if mine[key] != theirs[key]:
                raise ValueError(f"KDTrainStep.load_state_dict: the file was written by optimizer {theirs['kind']!r} (momentum "
                                 f"{theirs['momentum']}, nesterov {theirs['nesterov']}), this step runs {mine['kind']!r} (momentum "
                                 f"{mine['momentum']}, nesterov {mine['nesterov']}); their state does not carry over")
        ema = sd.get("ema") or {"kinds": [], "decays": []}
        if list(ema["kinds"]) != self.ema_kinds or [float(d) for d in ema["decays"]] != self.ema_decays:
            raise ValueError(f"KDTrainStep.load_state_dict: the file holds the EMA copies {list(zip(ema['kinds'], ema['decays']))}, "
                             f"this step keeps {list(zip(self.ema_kinds, self.ema_decays))}")

    def state_dict(self):
        """Everything that says where this QAT run stands, as host tensors and plain Python values: the arena (parameters, Adam moments
        and clocks), the host state of every quantizer by module path (activation: n_iter, observer_mode, sign; weight: observer_mode),
        _ranges_synced, the learning rate, the student's buffers and the parameters the arena does not hold (requires_grad False).
        While the ranks' activation ranges differ, every rank's ranges and n_iter travel too (`rank_ranges`, [world, quantizers, 3]
        int32 words: the bits of min and max, n_iter) -- which makes this a COLLECTIVE call at world > 1: every rank calls it, every rank
        gets the same `rank_ranges`.  Not stored: QuantTables, graphs and look-ahead results (rebuilt by the next eager quantizing step
        and maybe_capture), and the integer shadows of FQSS_DETERMINISTIC=1, which are empty between steps.  Nor the gradient
        accumulator: a window with micro-batches pending is refused (the trainers flush() before they write a checkpoint).
        Only a step that departs from plain Adam without decay adds `optim`; only a step with EMA copies adds `ema`."""
        if self.pending or self._open:
            raise RuntimeError(f"KDTrainStep.state_dict: {self.pending + int(self._open)} micro-batch(es) of an accumulation window are "
                               "pending; call flush() first (their gradients are not part of the stored state)")
        aqs, wqs = self._quantizers()
        if self._world() > 1 and any(getattr(m, "wants_output", False) and m.observing() for _, m in aqs):
            raise NotImplementedError("KDTrainStep.state_dict: inside the observer phase of act_observer: mse every rank holds its own "
                                      "histograms, which no file carries at world > 1; write the checkpoint after the first "
                                      f"{aqs[0][1].max_observations} steps (README, \"MSE activation observer\")")
        c = lambda t: t.detach().cpu().clone()
        held = {id(p) for p in self.arena.params}
        rank_ranges = None
        if self._ranks_differ() and aqs:
            mine = torch.stack([torch.cat([m.min_range.data.reshape(1), m.max_range.data.reshape(1)]).view(torch.int32) for _, m in aqs])
            mine = torch.cat([mine.cpu(), torch.tensor([[int(m.n_iter)] for _, m in aqs], dtype=torch.int32)], 1)
            rank_ranges = torch.stack(self.comm.all_gather(mine))
        more = {}
        if self._optim_block() is not None:
            more["optim"] = self._optim_block()
        if self.ema_decays:
            more["ema"] = {"kinds": list(self.ema_kinds), "decays": list(self.ema_decays), "count": c(self.ema_count),
                           "copies": [c(e) for e in self.ema], "extra": [{n: c(t) for n, t in x.items()} for x in self.ema_extra]}
        return {**more, "arena": self.arena.state_dict(),
                "act_quantizers": {n: {"n_iter": int(m.n_iter), "observer_mode": bool(m.observer_mode), "sign": bool(m.sign)} for n, m in aqs},
                "weight_quantizers": {n: {"observer_mode": bool(m.observer_mode)} for n, m in wqs},
                "ranges_synced": bool(self._ranges_synced), "lr": float(self.lr), "world": int(self._world()),
                "rank_ranges": rank_ranges,
                "buffers": {n: c(b) for n, b in self.model.named_buffers()},
                "frozen": {n: c(p) for n, p in self.model.named_parameters() if id(p) not in held}}

    def load_state_dict(self, sd):
        """into a step built like the one that was stored (same model structure, any fresh initialisation).  A file written while the
        ranks' ranges differed resumes at the SAME world size only, each rank taking its own ranges and n_iter; any other file serves
        any world size and any `buckets` (the arena is loaded by parameter name, whatever order the gradient buckets gave it).  Tables, graphs and look-ahead state are dropped: the next step runs eagerly, rebuilds the QuantTables (and
        starts no Adam clock again -- t0 is restored), and maybe_capture records the graphs afresh."""
        self._check_stored_optim(sd)
        aqs, wqs = self._quantizers()
        for kind, have, want in (("activation", aqs, sd["act_quantizers"]), ("weight", wqs, sd["weight_quantizers"])):
            if [n for n, _ in have] != list(want):
                odd = sorted(set(want) ^ {n for n, _ in have})
                raise ValueError(f"KDTrainStep.load_state_dict: the stored {kind} quantizers are not this model's "
                                 f"({len(want)} in the file, {len(have)} here; e.g. {odd[:3]})")
        rr = sd.get("rank_ranges")
        if rr is not None and int(sd["world"]) != self._world():
            raise ValueError(f"KDTrainStep.load_state_dict: this state was written at world size {int(sd['world'])} while the ranks still "
                             f"held their own observer ranges; it resumes at that world size only, not at {self._world()}")
        for n, m in aqs:
            if getattr(m, "wants_output", False):       # MSE observer: its histograms travel inside the observer phase and are gone after it
                m.set_scratch(f"{n}._hist" in sd["buffers"])
        buffers, frozen = dict(self.model.named_buffers()), {n: p for n, p in self.model.named_parameters()}
        for kind, have, want in (("buffers", buffers, sd["buffers"]), ("frozen parameters", frozen, sd["frozen"])):
            bad = [n for n, t in want.items() if n not in have or have[n].shape != t.shape]
            if bad or (kind == "buffers" and set(have) != set(want)):
                raise ValueError(f"KDTrainStep.load_state_dict: the stored {kind} are not this model's (e.g. {(bad or sorted(set(have) ^ set(want)))[:3]})")
        self.arena.load_state_dict(sd["arena"])
        if self.ema_decays:
            # the copies share the arena's layout: one written under another parameter order is gathered by name, like the arena
            mine, theirs = self.arena.layout(), sd["arena"]["layout"]
            at = dict(zip(theirs["names"], theirs["offsets"]))
            with torch.no_grad():
                for k, src in enumerate(sd["ema"]["copies"]):
                    if mine != theirs:
                        dst = torch.zeros(self.arena.numel, dtype=src.dtype)
                        for n, o, m in zip(mine["names"], mine["offsets"], mine["numel"]):
                            dst[o:o + m] = src[at[n]:at[n] + m]
                        src = dst
                    self.ema[k].copy_(src)
                    for n, t in sd["ema"]["extra"][k].items():
                        self.ema_extra[k][n].copy_(t)
                self.ema_count.copy_(sd["ema"]["count"])
        with torch.no_grad():
            for n, t in sd["buffers"].items():
                buffers[n].copy_(t)
            for n, t in sd["frozen"].items():
                frozen[n].data.copy_(t)
            if rr is not None:
                own = rr[self.comm.rank]
                for i, (_, m) in enumerate(aqs):
                    m.min_range.data.copy_(own[i, 0:1].view(torch.float32))
                    m.max_range.data.copy_(own[i, 1:2].view(torch.float32))
        for i, (n, m) in enumerate(aqs):
            q = sd["act_quantizers"][n]
            m.n_iter, m.observer_mode, m.sign = int(q["n_iter"] if rr is None else rr[self.comm.rank][i, 2]), bool(q["observer_mode"]), bool(q["sign"])
            m._fqss_deferred = False        # (a step that had tables: its range gradients are flushed per module until new tables exist)
        for n, m in wqs:
            m.observer_mode = bool(sd["weight_quantizers"][n]["observer_mode"])
        self.lr = float(sd["lr"])
        # is the one-time averaging of the observer ranges still due?
        if not (self._sync_ranges and self._exchange()):
            self._ranges_synced = True              # one rank, or a launch that declined the synchronisation: never
        elif rr is not None:
            self._ranges_synced = False             # the file holds per-rank ranges: the ranks differ until the phase ends
        elif not self.can_capture():
            self._ranges_synced = False             # one copy written INSIDE the observer phase (a world-1 file): the ranks part ways from here
        else:
            # one copy written past the phase: a world-N file says whether its ranks had averaged (True by then); a world-1 file says
            # True, and every rank starts from its identical ranges -- nothing to average
            self._ranges_synced = bool(sd["ranges_synced"])
        self.tables, self._graphs, self._graph_all, self._tgraph, self._ahead, self._ahead_key = None, None, None, None, None, None
        self._eager_q, self._odd, self.last = 0, 0, None
        self._pos, self._kept, self._open, self._win_eager = 0, 0, False, False      # (whatever window was open here is abandoned)

    def can_capture(self):
        from .quantization.qat.qat_quant import GradientActivationFakeQuantize, GradientWeightFakeQuantize
        for m in self.model.modules():
            if isinstance(m, GradientActivationFakeQuantize) and m.observing():
                return False
            if isinstance(m, GradientWeightFakeQuantize) and m.observer_mode:
                return False
        return True

    def maybe_capture(self, x, tgt):
        """training loops: once the observer phase is over (and after every learning-rate change) record the step into hipGraphs
        WITHOUT running it (warmup=0: no extra optimizer step); later calls with same-shaped batches replay.  At least one
        quantizing-phase step must have run eagerly first: it builds the QuantTables and starts the Adam clocks of the activation
        ranges (the captured clip+Adam launch does not activate parameters).  accumulate > 1: recorded at a window boundary only"""
        if self.use_graph and self._graphs is None and self._eager_q >= 1 and self.can_capture() and not (self._pos or self._open):
            self.capture(x, tgt, warmup=0)
        elif self._graphs is not None and not self._fits(x, tgt):
            # a batch of another shape (a file-backed loader's short utterance) runs eagerly (__call__); only when the NEW shape stays
            # (three steps in a row) are the graphs dropped and recorded again -- a capture costs seconds, an eager step milliseconds
            self._odd = getattr(self, "_odd", 0) + 1
            if self._odd >= 3:
                self._graphs, self._odd = None, 0
        elif self._graphs is not None:
            self._odd = 0

    def _fits(self, x, tgt):
        return x.shape == self._sx.shape and tgt.shape == self._st.shape

    # ---- the two halves of a step -----------------------------------------------------------
    def _take_ahead(self, x):
        """the teacher output the previous step computed for exactly this mixture tensor, or None"""
        ah, self._ahead = self._ahead, None
        if ah is not None and ah[0] is x and ah[1] == x._version:
            return ah[2]
        return None

    def _forward_loss(self, x, tgt, x_next=None, fest_given=None, join_teacher=True):
        """zero the gradient arenas, weight fake-quants, student + teacher forward, loss and dloss/dest -> (res, est, gest, cuts).
        fest_given: the teacher's output for x, already computed (look-ahead); x_next: start the teacher on the next mixture now"""
        a = self.arena
        a.zero_grad()
        t = self._quant_tables()
        if t is not None:
            t.gwq.zero_()
            t.weights_forward()                # all 101 weight fake-quants (+ int8 codes): one launch
        # The frozen teacher depends on nothing but x: it runs on a second stream next to the student's forward (its
        # MFMA-bound GEMMs overlap the student's HBM-bound layers; inside a hipGraph capture this becomes a parallel
        # branch of the graph) and joins before the loss.
        cur = None if self.cpu else torch.cuda.current_stream()
        teacher_free = self.loss_kind != "l1_sdr" and not self.kd_lambda > 0        # kd_lambda = 0: plain PIT SI-SDR loss, no teacher
        ahead = fest_given is not None
        two_streams = TEACHER_STREAM and not self.cpu
        if teacher_free:
            fest = None
        elif ahead:
            fest = fest_given
            if self._tstream is not None and join_teacher:      # computed on the teacher stream during the previous step (joined BEFORE the next look-ahead is enqueued there)
                cur.wait_stream(self._tstream)
                fest.record_stream(cur)
        elif two_streams:
            if self._tstream is None:
                self._tstream = _teacher_stream()
            self._tstream.wait_stream(cur)
            with torch.cuda.stream(self._tstream):
                fest = self.teacher(x)
        if x_next is not None and not teacher_free:
            # look-ahead: the next step's teacher forward, enqueued behind this step's own (if any) on the teacher stream; nothing in
            # this step waits for it -- the step that consumes it does
            if self._tstream is None:
                self._tstream = _teacher_stream()
            self._tstream.wait_stream(cur)
            with torch.cuda.stream(self._tstream):
                self._ahead = (x_next, x_next._version, self.teacher(x_next))
        cuts = []
        with ops.fast_codes(self.fast), ops.coded_dataflow(self.coded), ops.deferred(t):   # student: codes-only dataflow between quantizing layers
            if self.segments is not None:
                with ops.cut_recorder() as cuts:
                    est = self.model(x)
            else:
                est = self.model(x)
        if teacher_free or ahead:
            pass
        elif two_streams:
            cur.wait_stream(self._tstream)
            fest.record_stream(cur)
        else:
            fest = self.teacher(x)
        if self.loss_kind == "l1_sdr":
            if self.source_weights is None:
                self.source_weights = torch.ones(tgt.shape[1], device=tgt.device)
            loss, task, kd, w, gest = K.hd_kd_loss(est.detach(), fest, tgt, self.source_weights, self.kd_lambda, want_grad=True)
            if self.grad_at is not None:       # tests: dloss/dest taken at a given output (the L1 loss has a sign gradient)
                gest = K.hd_kd_loss(self.grad_at, fest, tgt, self.source_weights, self.kd_lambda, want_grad=True)[4]
            res = dict(loss=loss, task=task, kd=kd, w=w, gnorm=a.gnorm, est=est.detach())
        elif teacher_free:
            # mysystem.py:153-156: PITLossWrapper(pairwise_neg_sisdr) on the student alone
            out, sisdr, gest = K.pit_sisdr_loss(est.detach(), tgt, want_grad=True)
            res = dict(loss=out[0], kd_loss=out[1], task=out[2], kd=out[3], w=None, sisdr=sisdr, gnorm=a.gnorm, est=est.detach())
        else:
            # "sisdr_pit_per_sample": the speechbrain env's objective (log per sample, thresholded mean; csrc/train_ops.hip)
            out, w, sisdr, gest = K.kd_loss(est.detach(), fest, tgt, self.kd_lambda, want_grad=True,
                                            per_sample=self.loss_kind == "sisdr_pit_per_sample", threshold=self.loss_threshold)
            res = dict(loss=out[0], kd_loss=out[1], task=out[2], kd=out[3], w=w, sisdr=sisdr, gnorm=a.gnorm, est=est.detach())
        return res, est, gest, cuts

    def _backward_segment(self, k, est, gest, cuts):
        """backward segment k (k = 0: the END of the network ... k = len(cuts): its start) + that segment's quantizer finish"""
        t = self.tables
        regular = [c for c in cuts if not c[2]]
        nseg = len(regular) + 1
        if self.det is not None:
            if not torch.cuda.is_current_stream_capturing():
                self.det.activate()     # (no-op unless another step's DetMode has taken the device-wide control block since)
            if k == 0:
                self.det.begin_backward()
        with ops.deferred(t):
            if k == 0:
                est.backward(gest)
            else:
                roots = [regular[nseg - 1 - k]] + ([c for c in cuts if c[2]] if k == nseg - 1 else [])
                pairs = [(o, l.grad) for orig, leaves, _ in roots for o, l in zip(orig, leaves)
                         if o is not None and o.requires_grad and l.grad is not None]
                torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
        if t is not None:
            t.finish_backward(None if nseg == 1 else nseg - 1 - k)     # weight STE + range/slope gradients of this segment
        if self.det is not None:
            self.det.finish(0)      # the integer sums of this segment's bias / row-sum gradients -> the fp32 arena, before its exchange

    def _fwd_bwd(self, x, tgt, x_next=None, fest_given=None):
        """fwd + loss + the whole backward, no exchange (single rank; tests)"""
        res, est, gest, cuts = self._forward_loss(x, tgt, x_next, fest_given)
        for k in range(self._nseg(cuts)):
            self._backward_segment(k, est, gest, cuts)
        return res

    @staticmethod
    def _nseg(cuts):
        return sum(1 for c in cuts if not c[2]) + 1

    def _reduce_segment(self, k, nseg):
        """all-reduce(SUM) the gradient slice of backward segment k on the communication stream, behind everything enqueued on the
        current stream so far (RCCL over xGMI; the 1/world factor is folded into the clip+Adam kernel)"""
        if not self._exchange():
            return
        lo, hi = (0, self.arena.numel) if self.segments is None or nseg == 1 else self.segments[nseg - 1 - k]
        if self._cstream is None:
            self._cstream = torch.cuda.Stream()
        self._cstream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._cstream):
            self.comm.all_reduce_sum(self.arena.flat_g[lo:hi])

    def _join_reduces(self):
        if self._exchange() and self._cstream is not None:
            torch.cuda.current_stream().wait_stream(self._cstream)

    def _quant_tables(self):
        """batched per-quantizer work becomes available once every observer has finished"""
        if not self.batched_quantizers:
            return None
        if self.tables is None:
            from .quantization.qat.qat_quant import GradientActivationFakeQuantize, GradientWeightFakeQuantize
            for m in self.model.modules():
                if isinstance(m, GradientActivationFakeQuantize) and m.observing():
                    return None
                if isinstance(m, GradientWeightFakeQuantize) and m.observer_mode:
                    return None
            self.tables = QuantTables(self.model, self.arena, segments=self._seg_ids)
            if self.det is not None:
                self.det.attach(1, self.tables.gwq)
                self.tables.det = self.det
        return self.tables

    def _world(self):
        return self.comm.world if self.comm is not None else 1

    def _exchange(self):
        """collectives are issued: world > 1, or a forced one-rank communicator (parallel.Comm.force)"""
        return self.comm is not None and getattr(self.comm, "active", self.comm.world > 1)

    def _optimize(self, activate=True):
        if activate:
            self.arena._activate_touched()
        # the update takes the average of the gradients it is given: over the ranks and over the micro-batches of a window
        o = self.optim
        self.arena.clip_optim_step(self.lr, self.clip, 1.0 / (self._world() * self.accumulate), betas=self.betas, activate=False,
                                   kind=o["kind"], weight_decay=o["weight_decay"], momentum=o["momentum"], nesterov=o["nesterov"],
                                   wd_slot=self._wd_slot)
        # the batch-level EMA copies follow every update (solver.py:425-427), every rank computing the same average
        for k, kind in enumerate(self.ema_kinds):
            if kind == "batch":
                self._ema_update(k)

    # ---- EMA copies of the model (demucs' ModelEMA; fqss.h: fqss_ema_update) --------------------------------------------------
    def _ema_update(self, k):
        """one launch over the whole arena; w = 1 / count comes from the device-resident count, which the launch advances -- so the
        update may sit inside a captured graph.  The float32 state_dict entries outside the arena follow with torch ops on the same
        device word"""
        count = self.ema_count[k:k + 1]
        K.ema_update(self.ema[k], self.arena.flat_p, decay=self.ema_decays[k], count=count)
        if self._ema_outside:
            w = (1.0 / count).to(torch.float32)
            for n, t in self._ema_outside:
                self.ema_extra[k][n].mul_(1.0 - w).add_(t.detach() * w)

    def ema_epoch_update(self):
        """the epoch-level copies, once per epoch after training (solver.py:438-440)"""
        for k, kind in enumerate(self.ema_kinds):
            if kind == "epoch":
                self._ema_update(k)

    def ema_state(self, k):
        """copy k shaped like model.state_dict(): views of the copy for the arena's parameters, the copy's own tensors for the other
        float32 entries, the model's entries for whatever is not float32 (ModelEMA keeps float32 entries only)"""
        at = {id(p): (o, p) for p, o in zip(self.arena.params, self.arena.offsets)}
        out = {}
        for n, t in self.model.state_dict(keep_vars=True).items():
            if id(t) in at:
                o, p = at[id(t)]
                out[n] = self.ema[k][o:o + p.numel()].view(p.shape)
            elif n in self.ema_extra[k]:
                out[n] = self.ema_extra[k][n]
            else:
                out[n] = t.detach()
        return out

    def ema_swap(self, k):
        """context manager: the model computes with copy k inside, with its own parameters again after.  The exchange is device to
        device INTO the arena's buffer, so p.data keeps its address and graphs and device tables stay valid"""
        import contextlib

        def exchange():
            with torch.no_grad():
                pairs = [(self.arena.flat_p, self.ema[k])] + [(t.detach(), self.ema_extra[k][n]) for n, t in self._ema_outside]
                for a, b in pairs:
                    tmp = a.clone()
                    a.copy_(b)
                    b.copy_(tmp)

        @contextlib.contextmanager
        def swapped():
            exchange()
            try:
                yield self
            finally:
                exchange()
        return swapped()

    def _maybe_sync_ranges(self):
        """world > 1: once, when the observer phase is over, every rank takes the mean of the observed activation ranges"""
        if not self._ranges_synced and self.can_capture():
            self.comm.sync_observer_ranges(self.model)
            self._ranges_synced = True

    def _step_eager(self, x, tgt, x_next=None, exchange=True):
        """fwd + loss, then per backward segment: backward -> all-reduce of its gradient slice on the communication stream, which
        overlaps the next segment's backward; the optimizer waits for the last exchange.  exchange=False (a micro-batch of an
        accumulation window): no collective -- the window's sum is exchanged once, by commit() / flush()"""
        fest = self._take_ahead(x) if self.teacher_ahead else None
        res, est, gest, cuts = self._forward_loss(x, tgt, x_next if self.teacher_ahead else None, fest)
        nseg = self._nseg(cuts)
        for k in range(nseg):
            self._backward_segment(k, est, gest, cuts)
            if exchange:
                self._reduce_segment(k, nseg)
        if exchange:
            self._join_reduces()
        return res

    # ---- gradient accumulation: a window of `accumulate` micro-batches per update (DESIGN.md "Gradient accumulation") ---------
    @property
    def pending(self):
        """micro-batches of the open window, kept or dropped (0: the last call ended with an update, or nothing has run)"""
        return self._pos

    def micro_batch(self, x, tgt, x_next=None):
        """first half of a call: fwd + loss + bwd of one micro-batch into the gradient arena (hipGraph replay where the graphs fit).
        Nothing is exchanged, accumulated or updated before commit() says whether this micro-batch counts."""
        if self._open:
            raise RuntimeError("KDTrainStep.micro_batch: the previous micro-batch has not been committed")
        self._maybe_sync_ranges()
        if self._graphs is not None and self.use_graph and self._fits(x, tgt):
            r = self.replay_fwd_bwd(x, tgt, x_next if (x_next is not None and x_next.shape == x.shape) else None, exchange=False)
        else:
            self.last = r = self._step_eager(x, tgt, x_next, exchange=False)
            self._win_eager = True
        self._open = True
        return r

    def commit(self, keep=True):
        """second half: keep=True adds the micro-batch's gradient to the window, keep=False drops it; either way the window moves on
        and its divisor stays world * accumulate.  The last micro-batch of a window brings the sum into the gradient arena, exchanges
        it and updates -- unless every micro-batch was dropped: then nothing is updated and no Adam clock moves.  At world > 1 every
        rank passes the same `keep` (the exchange is a collective).  True when an update ran."""
        if not self._open:
            raise RuntimeError("KDTrainStep.commit: no micro-batch to commit")
        self._open = False
        a = self.arena
        last = self._pos + 1 == self.accumulate
        if last:
            # kept, with earlier ones held: g += acc; dropped: g = acc; kept and alone: g is the sum already
            mode = (K.ACC_FINISH if keep else K.ACC_TAKE) if self._kept else None
            return self._end_window(mode, update=bool(keep or self._kept))
        if keep:
            K.grad_accum(a.acc, a.flat_g, K.ACC_ADD if self._kept else K.ACC_SET)      # (the first kept one needs no zeroed accumulator)
            self._kept += 1
        self._pos += 1
        return False

    def flush(self):
        """end the open window early (end of an epoch, before validation and the checkpoint): the held sum is exchanged and applied at
        the same 1 / (world * accumulate) -- each micro-batch's share was fixed when it ran, as under pl.Trainer.  Nothing pending:
        nothing happens.  True when an update ran."""
        if self._open:
            raise RuntimeError("KDTrainStep.flush: the last micro-batch has not been committed")
        if self._pos == 0:
            return False
        return self._end_window(K.ACC_TAKE if self._kept else None, update=self._kept > 0)

    def _end_window(self, mode, update):
        """the window's sum into the gradient arena (fqss_grad_accum `mode`; None: it is there already), slice by slice in the order the
        backward segments finish, each slice's all-reduce on the communication stream behind its own launch (it overlaps the next
        slice's); then clip + Adam on the averaged sum"""
        a = self.arena
        if update:
            nseg = len(self.segments) if self.segments is not None else 1
            for k in range(nseg):
                lo, hi = (0, a.numel) if nseg == 1 else self.segments[nseg - 1 - k]
                if mode is not None:
                    K.grad_accum(a.acc[lo:hi], a.flat_g[lo:hi], mode)
                self._reduce_segment(k, nseg)
            self._join_reduces()
            if self._graphs is not None and not self._win_eager:
                self.replay_optimize()
            else:
                self._optimize()
                if self.tables is not None or (not self.batched_quantizers and self.can_capture()):
                    self._eager_q += 1
        self._pos, self._kept, self._win_eager = 0, 0, False
        return update

    def __call__(self, x, tgt, x_next=None):
        """x_next (teacher_ahead=True only): the mixture tensor the NEXT call will be given -- the same tensor object, unmodified.
        accumulate > 1: one micro-batch; the call that completes a window also updates (`pending` is 0 after it)"""
        if self.accumulate > 1:
            r = self.micro_batch(x, tgt, x_next)
            self.commit()
            return r
        self._maybe_sync_ranges()
        if self._graphs is not None and self.use_graph and self._fits(x, tgt):
            return self.replay(x, tgt, x_next if (x_next is not None and x_next.shape == x.shape) else None)
        self.last = self._step_eager(x, tgt, x_next)
        self._optimize()
        if self.tables is not None or (not self.batched_quantizers and self.can_capture()):
            self._eager_q += 1
        return self.last

    # ---- hipGraph capture -------------------------------------------------------------------
    def capture(self, x, tgt, warmup=2):
        # a prefetching loader's reader thread allocates and launches on its own stream: not while this thread records a graph (the
        # default capture mode faults on another thread's hipMalloc / event calls)
        from .loader import DEVICE_WORK_LOCK
        if self._pos or self._open:
            raise RuntimeError("KDTrainStep.capture: an accumulation window is open; graphs are recorded at a window boundary")
        with DEVICE_WORK_LOCK:
            return self._capture(x, tgt, warmup)

    def _capture(self, x, tgt, warmup=2):
        from .quantization.qat.qat_quant import GradientActivationFakeQuantize, GradientWeightFakeQuantize
        for m in self.model.modules():
            if isinstance(m, GradientActivationFakeQuantize):
                assert not m.observing(), "capture() needs the observer phase to be over"
            if isinstance(m, GradientWeightFakeQuantize):
                assert not m.observer_mode, "capture() needs the weight observers to have run"
        self._maybe_sync_ranges()
        self._own_det()         # (another step of this process may have run since this one's last eager call)
        self._sx, self._st = x.clone(), tgt.clone()
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(warmup):              # eager steps: activates every live parameter's Adam clock (bench: warm caches)
                if self.accumulate > 1:          # ... whole windows of them
                    for _ in range(self.accumulate):
                        self.last = self._step_eager(self._sx, self._st, exchange=False)
                        self._open = self._win_eager = True
                        self.commit()
                    continue
                self.last = self._step_eager(self._sx, self._st)
                self._optimize()
        cur.wait_stream(side)
        torch.cuda.synchronize()
        # one hipGraph per backward segment (the first also holds fwd + loss) and one for clip + Adam: at world > 1 the exchange of
        # a segment's gradients is launched between two replays and overlaps the next one (no collective inside a graph)
        # (at world > 1 the process group's watchdog thread polls its events while this thread captures: only THIS thread's calls are
        # checked against the capture then -- torch's default mode lets a query from any thread invalidate it)
        mode = dict(capture_error_mode="thread_local") if self._exchange() else {}
        # teacher_ahead: the teacher's forward is a graph of its OWN (own memory pool: it replays on the teacher stream WHILE the step's
        # graphs replay) from the static look-ahead mixture _sxn into _fest_next; the step's graphs read the static copy _fest_cur
        fest_cur = None
        self._tgraph = None
        self._ahead_key = None
        if self.teacher_ahead and (self.loss_kind == "l1_sdr" or self.kd_lambda > 0):
            if self._tstream is None:
                self._tstream = _teacher_stream()
            self._sxn = x.clone()
            tg = torch.cuda.CUDAGraph()
            self._tstream.wait_stream(cur)
            with torch.cuda.graph(tg, stream=self._tstream, **mode):
                self._fest_next = self.teacher(self._sxn)
            cur.wait_stream(self._tstream)
            self._fest_cur = fest_cur = torch.empty_like(self._fest_next)
            self._tgraph = tg
        graphs = [torch.cuda.CUDAGraph()]
        with torch.cuda.graph(graphs[0], **mode):
            self.last, est, gest, cuts = self._forward_loss(self._sx, self._st, None, fest_cur, False)
            self._backward_segment(0, est, gest, cuts)
        for k in range(1, self._nseg(cuts)):
            gk = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gk, pool=graphs[0].pool(), **mode):
                self._backward_segment(k, est, gest, cuts)
            graphs.append(gk)
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, pool=graphs[0].pool(), **mode):
            self._optimize(activate=False)
        self._graphs = (graphs, g2)
        del est, gest, cuts
        # single rank, one segment: nothing has to happen between the two halves, so the whole step is ALSO captured as one graph
        # (replay() then costs one launch; replay_fwd_bwd / replay_optimize keep serving the trainers that may skip an update)
        # (accumulate > 1: an accumulate launch, and on most micro-batches no update, sits between the halves -- the two-graph form serves)
        self._graph_all = None
        if not self._exchange() and len(graphs) == 1 and self.accumulate == 1:
            ga = torch.cuda.CUDAGraph()
            with torch.cuda.graph(ga, pool=graphs[0].pool()):
                self.last_all, est, gest, cuts = self._forward_loss(self._sx, self._st, None, fest_cur, False)
                self._backward_segment(0, est, gest, cuts)
                self._optimize(activate=False)
            self._graph_all = ga
            del est, gest, cuts
        return self

    def _stage(self, x, tgt, x_next):
        """inputs of a replay into the static buffers; teacher_ahead: hand the teacher output of this mixture (the previous replay's
        look-ahead, or a teacher replay right now if nobody announced the mixture) to the step's graphs, then start the teacher graph
        on the next mixture on the teacher stream"""
        if self._tgraph is None:
            if x is not None and x.data_ptr() != self._sx.data_ptr():
                self._sx.copy_(x)
                self._st.copy_(tgt)
            return
        cur, ts = torch.cuda.current_stream(), self._tstream
        src = self._sx if x is None else x
        key = self._ahead_key
        if not (key is not None and key[0] is src and key[1] == src._version):
            eager = self._take_ahead(src)          # an eager step (before the capture) may have looked ahead for this mixture
            ts.wait_stream(cur)
            with torch.cuda.stream(ts):
                if eager is not None:
                    self._fest_next.copy_(eager)
                else:
                    if src.data_ptr() != self._sxn.data_ptr():
                        self._sxn.copy_(src)
                    self._tgraph.replay()
        cur.wait_stream(ts)
        self._fest_cur.copy_(self._fest_next)
        if x is not None and x.data_ptr() != self._sx.data_ptr():
            self._sx.copy_(x)
            self._st.copy_(tgt)
        self._ahead_key = None
        if x_next is not None:
            self._sxn.copy_(x_next)
            ts.wait_stream(cur)
            with torch.cuda.stream(ts):
                self._tgraph.replay()
            self._ahead_key = (x_next, x_next._version)

    def _own_det(self):
        """FQSS_DETERMINISTIC=1: the device-wide control block must point at THIS step's shadows while its graphs replay -- another step's
        activate() since the capture would leave the replayed grad_adds on plain fp32 atomics without a word"""
        if self.det is not None and K.DetMode.owner is not self.det:
            self.det.activate()

    def replay_fwd_bwd(self, x=None, tgt=None, x_next=None, exchange=True):
        """first half of a captured step (fwd + loss + bwd, gradients exchanged); the caller then calls replay_optimize() or skips.
        exchange=False (a micro-batch of an accumulation window): no collective is due here, commit() / flush() issue the window's"""
        self._own_det()
        self._stage(x, tgt, x_next)
        graphs = self._graphs[0]
        ev = self.comm_events
        for k, gk in enumerate(graphs):
            gk.replay()
            if ev is not None and k == len(graphs) - 1:
                ev[0].record()                  # the backward is over: whatever the optimizer still waits for is exposed exchange time
            if exchange:
                self._reduce_segment(k, len(graphs))
        if exchange:
            self._join_reduces()
        if ev is not None:
            ev[1].record()
        return self.last

    def replay_optimize(self):
        self.arena._host_step += 1
        self._graphs[1].replay()

    def replay(self, x=None, tgt=None, x_next=None):
        if self.accumulate > 1:
            # one micro-batch; the one that completes the window also exchanges and replays clip + Adam (commit)
            if self._open:
                raise RuntimeError("KDTrainStep.replay: the previous micro-batch has not been committed")
            r = self.replay_fwd_bwd(x, tgt, x_next, exchange=False)
            self._open = True
            self.commit()
            return r
        if getattr(self, "_graph_all", None) is not None:
            self._own_det()
            self._stage(x, tgt, x_next)
            self.arena._host_step += 1
            self._graph_all.replay()
            return self.last_all
        self.replay_fwd_bwd(x, tgt, x_next)
        self.replay_optimize()
        return self.last


class InferRunner:
    """Quantized inference as it would be served: the eval-mode forward on the codes-only dataflow
    (activations travel between layers as u8 codes, the 1x1 convolutions run on the integer codes: bit-identical to the plain eval
    forward) captured into one hipGraph per input shape, so a request costs one graph launch."""

    def __init__(self, model, use_graph=True):
        from .quantization.qat.models.load_model import enable_observer
        self.model = model.eval()
        enable_observer(self.model, False)
        self.use_graph = use_graph
        self._graphs = {}
        if hasattr(model, "n_srcs"):
            self.n_srcs = model.n_srcs         # process.model_infer asks its `model` for it

    @torch.no_grad()
    def _forward(self, x):
        with ops.fast_codes(True):
            return self.model(x)

    @torch.no_grad()
    def __call__(self, x):
        if not self.use_graph:
            return self._forward(x)
        key = tuple(x.shape) + (ops.SPLIT_PER_ITEM,)     # per-item and global splitter: two graphs of one shape, never each other's
        ent = self._graphs.get(key)
        if ent is None:
            sx = x.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):                      # warm-up outside the capture (allocator, lazy tables)
                    self._forward(sx)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = self._forward(sx)
            ent = self._graphs[key] = (g, sx, out)
        g, sx, out = ent
        if x.data_ptr() != sx.data_ptr():
            sx.copy_(x)
        g.replay()
        return out
