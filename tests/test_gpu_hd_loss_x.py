"""GPU: fqss_hd_loss_x (csrc/hd_loss.hip -> kernels.hd_loss_x) against the float64 restatement of tests/helpers_hd_loss_x.py, which
states the shapes, the gates and the MI355X measurements behind them."""
import pytest
import torch

from tests import helpers_hd_loss_x as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", H.SHAPES, ids=str)
@pytest.mark.parametrize("want_grad", [True, False])
@pytest.mark.parametrize("kind,teacher", H.MODES)
def test_hd_loss_x_against_fp64(kind, teacher, want_grad, shape):
    H.check_case(kind, teacher, shape, want_grad, "cuda")


def test_hd_loss_x_refusals():
    H.check_refusals("cuda")


@pytest.mark.parametrize("kind,teacher", H.MODES)
def test_hd_loss_x_same_bits_on_two_streams(kind, teacher):
    """no atomics: two runs on two streams, and the one-sample load form (a copy one float off 16-byte alignment), give the same bits"""
    from fqss_amd import kernels as K
    est, fest, src, wt, lam = H.case(4, 4, 2 * H.TILE + 1028, teacher=teacher, device="cuda")       # N % 4 == 0: the 16-byte form

    def shifted(t):
        return None if t is None else torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)

    runs = []
    for ops in ((est, fest, src), (est, fest, src), tuple(shifted(t) for t in (est, fest, src))):
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            r = K.hd_loss_x(ops[0], ops[1], ops[2], wt, lam, kind=kind)
        st.synchronize()
        runs.append(torch.cat([t.reshape(-1) for t in r]))
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
