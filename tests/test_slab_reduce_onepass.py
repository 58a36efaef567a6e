"""The fp32 slab reduce of the split-K weight gradients (conv_wgrad.hip launch_reduce; lib.slab_reduce): one
launch for small outputs too -- row groups summed by the row lanes of a workgroup, combined through LDS in a fixed
order -- against a float64 sum, bit-repeatable, and with the slab left untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
_MANT = {torch.float16: 10, torch.bfloat16: 7}


def _lib():
    from mxnet_maintenance_amd.ops import kernels
    assert kernels.available(), 'HIP kernel extension not loaded: %s' % kernels.load_error()
    return kernels.lib()


def _half_ulp(ref, dtype):
    """Half the spacing of ``dtype`` at |ref| (float64 tensor)."""
    tiny = 2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126
    e = torch.frexp(ref.abs().clamp_min(tiny))[1].double()          # |ref| = m * 2^e, m in [0.5, 1)
    return 0.5 * torch.exp2(e - 1 - _MANT[dtype])


# n: 4 (one quad, as many row groups as rows), 4096 (the 64x64 weight, fewest workgroups), 16388 (a partly filled
# last workgroup), 262144 / 262148 (the largest 1x1 weight of ResNet-50 that is reduced with row lanes, and the
# first size that takes one thread per column quad), 524284 / 524288 (large outputs); splits: none to combine,
# fewer than the row lanes, odd, and more than one row per group
@pytest.mark.parametrize('n', [4, 4096, 16388, 262144, 262148, 524284, 524288])
@pytest.mark.parametrize('splits', [1, 2, 3, 16, 64, 67])
def test_slab_reduce_matches_float64(n, splits):
    lib = _lib()
    dev = 'cuda'
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev).manual_seed(n + splits)
    slab = torch.randn(splits, n, device=dev, generator=g)
    keep = slab.clone()
    ref_sum = slab.double().sum(0)
    abs_sum = slab.double().abs().sum(0)
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        for accum in (0, 1):
            prev = torch.randn(n, device=dev, generator=g).to(dtype)
            out = prev.clone()
            lib.slab_reduce(_DT[dtype], slab.data_ptr(), splits, n, out.data_ptr(), accum, st)
            ref = ref_sum + (prev.double() if accum else 0)
            bound = (splits + accum) * 2.0 ** -23 * (abs_sum + (prev.double().abs() if accum else 0))
            if dtype != torch.float32:
                bound = bound + _half_ulp(ref, dtype)
            excess = ((out.double() - ref).abs() - bound).max().item()
            assert excess <= 0, (dtype, accum, excess)
            # the order of the additions is fixed: a second call returns the same bits
            out2 = prev.clone()
            lib.slab_reduce(_DT[dtype], slab.data_ptr(), splits, n, out2.data_ptr(), accum, st)
            assert torch.equal(out.view(torch.int32 if dtype == torch.float32 else torch.int16),
                               out2.view(torch.int32 if dtype == torch.float32 else torch.int16))
    # the slab is only read (no in-place fold of row groups)
    assert torch.equal(slab, keep)


@pytest.mark.parametrize('cfg', [(2, 14, 64, 256, 1), (2, 7, 64, 64, 3)])
def test_conv_wgrad_through_the_reduce(cfg):
    """Weight gradients of a 1x1 and a 3x3 conv whose split-K slabs are small outputs, against fp32 torch."""
    from mxnet_maintenance_amd.ops import kernel_fns as KF
    _lib()
    N, H, Cin, Cout, k = cfg
    pad = k // 2
    dtype = torch.float16
    torch.manual_seed(2)
    x = torch.randn(N, H, H, Cin, device='cuda').to(dtype)
    w = torch.randn(Cout, k, k, Cin, device='cuda').to(dtype)
    dy = torch.randn(N, H, H, Cout, device='cuda').to(dtype)
    assert KF.conv_wgrad_ok(x, w)
    ref = torch.ops.aten.convolution_backward(
        dy.float().permute(0, 3, 1, 2), x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), None,
        [1, 1], [pad, pad], [1, 1], False, [0, 0], 1, [False, True, False])[1].permute(0, 2, 3, 1)
    tol = 2e-3                           # fp16, as test_hip_kernels.test_conv_wgrad_matches_fp32
    dw = KF.conv_wgrad(x, dy, w.shape, (1, 1), (pad, pad))
    assert float((dw.float() - ref).norm() / ref.norm()) < tol
    torch.testing.assert_close(dw.float(), ref, rtol=0, atol=tol * ref.abs().max().item())
    acc = torch.ones(Cout, k, k, Cin, device='cuda')
    KF.conv_wgrad(x, dy, w.shape, (1, 1), (pad, pad), out=acc, accum=True)
    assert float((acc - 1 - ref).norm() / ref.norm()) < tol
