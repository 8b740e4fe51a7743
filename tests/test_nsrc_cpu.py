"""The PIT / KD loss at one and three sources on the CPU backend (fqss_amd/csrc/cpu/libfqss_cpu.so: fqss_kd_loss_n,
fqss_kd_moments_n), against the reference-generated fixture tests/golden/nsrc_loss.npz (tools/make_goldens_nsrc.py) and the live
oracle; the wrapper's refusals; `data.synth_batch(n_src=)`; two steps of a tiny three-source ConvTasNetQ.  No GPU.
The bodies are tests/nsrc_common.py's, which tests/test_gpu_nsrc.py runs on the HIP kernels."""
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import fqss_oracle as O
from tests import nsrc_common as N

HOST = lambda t: t


@pytest.fixture()
def cpu_backend():
    from fqss_amd import _lib
    if not os.path.exists(_lib.CPU_SO_PATH):
        subprocess.check_call(["make", "-C", os.path.dirname(_lib.CPU_SO_PATH)])
    _lib.set_backend("cpu")
    yield
    _lib.set_backend("hip")


def test_three_source_loss_fixture(golden, cpu_backend):
    """all six permutations, the two 3-cycles among them (samples 3 and 4): loss, kd, task, w, SI-SDR, dL/d est"""
    from fqss_amd import kernels as K
    N.check_fixture(K, HOST, golden("nsrc_loss"))


@pytest.mark.parametrize("S", [3, 1])
def test_kd_loss_against_oracle(cpu_backend, S):
    from fqss_amd import kernels as K
    for B, T in ((6, 1000), (1, 257)):
        N.check_kd_loss(K, HOST, S, B, T)


@pytest.mark.parametrize("S", [3, 1])
def test_pit_sisdr_against_oracle(cpu_backend, S):
    from fqss_amd import kernels as K
    N.check_pit_sisdr(K, HOST, S, 6, 1000)


@pytest.mark.parametrize("S", [3, 1])
def test_per_sample_objective_against_oracle(cpu_backend, S):
    """B = 1 and B = n_src; at S = 3 once from sample 0 and once from sample 3 (both 3-cycles inside)"""
    from fqss_amd import kernels as K
    for first in ((0, 3) if S == 3 else (0,)):
        N.check_speechbrain(K, HOST, S, 1000, first=first)


@pytest.mark.parametrize("S", [3, 1])
def test_moments_and_evaluation_forms(cpu_backend, S):
    """fqss_kd_moments_n, and the evaluation forms that slice its table by S"""
    from fqss_amd import kernels as K
    from fqss_amd.train_env.asteroid_librimix import wsdr
    N.check_moments(K, HOST, S, 6, 1000)
    s, e, f = N.batch(S, 6, 1000)
    pw = wsdr.PairwiseWSDR("sisdr", take_log=True)(e, s)
    assert pw.shape == (6, S, S)
    np.testing.assert_allclose(pw.numpy(), O.pairwise_sisdr(e.double(), s.double(), take_log=True).numpy(), atol=1e-3)
    per = torch.stack([-O.neg_sisdr_pit(e[b:b + 1].double(), s[b:b + 1].double()) for b in range(6)])
    np.testing.assert_allclose(wsdr.si_sdr(e, s).numpy(), per.numpy(), atol=1e-3)
    diag = -torch.diagonal(O.pairwise_sisdr(e.double(), s.double()), dim1=1, dim2=2)
    np.testing.assert_allclose(float(wsdr.sisdr(e, s)), float(diag.mean()), rtol=1e-5)


def test_refusals(cpu_backend):
    from fqss_amd import _lib, kernels as K
    s, e, f = N.batch3(2, 300)
    with pytest.raises(_lib.FqssError, match="B must be 1 or n_src"):
        K.kd_loss(e, f, s, 0.1, per_sample=True)                     # three sources, batch 2
    x4 = torch.zeros(1, 4, 300)
    for call in (lambda: K.kd_loss(x4, x4, x4, 0.1), lambda: K.pit_sisdr_loss(x4, x4), lambda: K.kd_moments(x4, x4, x4)):
        with pytest.raises(NotImplementedError, match="1 to 3"):
            call()


def test_synth_batch_n_src():
    from fqss_amd import data
    x, s = data.synth_batch(3, 500, seed=7, n_src=2)
    xo, so = O.synth_batch(3, 500, seed=7)
    assert torch.equal(x, xo) and torch.equal(s, so)
    x0, s0 = data.synth_batch(3, 500, seed=7)
    assert torch.equal(x0, xo) and torch.equal(s0, so)
    x3, s3 = data.synth_batch(2, 500, seed=7, n_src=3)
    assert s3.shape == (2, 3, 500) and x3.shape == (2, 1, 500) and torch.equal(x3, s3.sum(1, keepdim=True))


def test_tiny_three_source_training(cpu_backend):
    N.check_tiny_training("cpu")


def test_dual_path_models_refuse_other_source_counts():
    from fqss_amd.quantization.qat.models.dptnetq import DPTNetQ
    from fqss_amd.quantization.qat.models.sepformerq import SepformerQ
    for make in (lambda: DPTNetQ(n_spks=3, kernel_size=2, enc_dim=16, feature_dim=8, hidden_dim=12, layer=2, segment_size=10),
                 lambda: SepformerQ(n_spks=3, kernel_size=16, stride=8, n_filters=16, n_repeats=1, n_heads=4, chunk_size=10)):
        with pytest.raises(NotImplementedError, match="n_spks = 2"):
            make()
