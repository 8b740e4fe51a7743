"""fqss_hd_loss_x on the CPU backend (fqss_amd/csrc/cpu/libfqss_cpu.so, `_lib.set_backend("cpu")`) against the float64 restatement of
tests/helpers_hd_loss_x.py: the shapes, gates and case body of the GPU test."""
import pytest
import torch

from tests import helpers_hd_loss_x as H


@pytest.fixture()
def cpu_backend():
    from fqss_amd import _lib
    _lib.set_backend("cpu")
    yield
    _lib.set_backend("hip")


@pytest.mark.parametrize("shape", H.SHAPES, ids=str)
@pytest.mark.parametrize("kind,teacher", H.MODES)
def test_cpu_backend_hd_loss_x_against_fp64(cpu_backend, kind, teacher, shape):
    H.check_case(kind, teacher, shape, True, "cpu")


def test_cpu_backend_hd_loss_x_refusals_and_empty_batch(cpu_backend):
    from fqss_amd import kernels as K
    H.check_refusals("cpu")
    est, _, src, wt, _ = H.case(2, 2, 64)
    empty = K.hd_loss_x(est[:0], None, src[:0], wt, 0.0)              # B = 0: FQSS_OK, nothing written -- the means of nothing are NaN
    assert empty.gest.numel() == 0 and all(bool(torch.isnan(getattr(empty, n)).all()) for n in H.FIELDS)
