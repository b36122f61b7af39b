"""The factor-and-invert family of csrc/dkt_lds_dense.h is ONE code: a row-noise problem whose rows all carry the noise of their class is the leave-one-out
kernel's problem at the first rung of its ladder, and both kernels run the same staging, sweep, inverse and row product on it -- alpha agrees bit for bit.
(The float64 sweeps of the two kernels are tests/test_dirichlet_gpu.py and tests/test_loo_gpu.py; this one only keeps the sharing honest.)"""
import pytest
import torch

from dkt_amd import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 17, 64, 65, 127])          # a single row; an odd size; the wave-half edge and either side of it; the largest problem
def test_rownoise_and_loo_share_alpha_bit_for_bit(n, cuda):
    b, c = 2, 2
    g = torch.Generator().manual_seed(1000 + n)
    z = torch.randn((b, n, n + 3), generator=g)
    e = (z @ z.transpose(-1, -2) / (n + 3)).contiguous().to(cuda)
    y = torch.randn((b, c, n), generator=g).to(cuda)
    sv = (0.5 + torch.rand((c,), generator=g)).to(cuda)
    mean = (0.1 * torch.randn((c,), generator=g)).to(cuda)
    noise = (0.05 + 0.1 * torch.rand((c,), generator=g)).to(cuda)
    noise_rows = noise.reshape(1, c, 1).expand(b, c, n).contiguous()
    rn = ops.mll_rownoise(e, y, noise_rows, sv, mean)
    lo = ops.loo(e, y, sv, mean, noise, max_tries=0)
    assert int(rn["info"].abs().max()) == 0 and int(lo["info"].abs().max()) == 0 and float(lo["jitter"].abs().max()) == 0.0
    assert torch.isfinite(rn["alpha"]).all()
    assert torch.equal(rn["alpha"].view(torch.int32), lo["alpha"].view(torch.int32))
