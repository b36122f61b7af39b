"""The product library carries the 64-row large-N Gram backward (`gram_bwd_rows_f16x2_kernel<KS, 4>`) only up to 256 rows: beyond, its dispatch always took
the 128-row kernel, and the `<10 | 12 | 14, 4>` instances nothing could launch are compiled for the twins library only (docs/MEASUREMENTS.md R12).  Nothing
may have changed for a caller: `dkt_gram_bwd_f32` of the product and of libdkt_twins.so (default switches) agree bit for bit at 256 < N <= 448."""
import ctypes

import pytest
import torch

import dkt_amd

pytestmark = pytest.mark.gpu
L = dkt_amd._lib


@pytest.mark.parametrize("b, n, d", [(3, 257, 64), (3, 300, 64), (2, 320, 512), (3, 384, 128), (2, 420, 512), (9, 447, 64), (2, 448, 68)])
def test_product_and_twins_gram_backward_agree_bitwise_beyond_256_rows(b, n, d, cuda, monkeypatch):
    for k in dkt_amd.ops._VARIANT_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    prod, twin = L.load(), L.load_twins()
    for lib in (prod, twin):
        L.reload_env(lib)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    g = torch.Generator(device="cuda").manual_seed(n)
    z = torch.nn.functional.normalize(torch.randn(b, n, d, device=cuda, generator=g), dim=2).contiguous()
    w = torch.randn(b, n, n, device=cuda, generator=g)
    w = (w + w.transpose(1, 2)).contiguous()
    outs = []
    for lib in (prod, twin):
        dz = torch.full_like(z, float("nan"))
        assert lib.dkt_gram_bwd_f32(p(w), p(z), p(dz), b, n, d, None, dkt_amd.ops.GRAM_UNIT_ROWS | dkt_amd.ops.GRAM_W_SYMMETRIC, None) == 0
        torch.cuda.synchronize()
        outs.append(dz)
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])
    ref = 2.0 * torch.bmm(w.double(), z.double())
    assert float((outs[0].double() - ref).abs().max()) < 1e-4 * float(ref.abs().max())
