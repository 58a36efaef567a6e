"""relu(BN(data) + BN_shortcut(shortcut_data)) as one operator (``_contrib_BatchNormBatchNormAddReLU``): the
residual tail that normalises a projection shortcut itself (bn_apply_kernel's affine addend,
kernel_fns.BatchNormDualTailNHWC) against the two-operator composition and an fp32 torch reference."""
import json
import os

import numpy as np
import pytest
import torch

import mxnet_maintenance_amd as mx
from mxnet_maintenance_amd import autograd, gluon, nd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resnet_fused_nhwc_param_names.json')


# ----------------------------------------------------------------------------- CPU

def _nd_inputs(ctx, shape, seed):
    rs = np.random.RandomState(seed)
    C = shape[-1]
    arrs = dict(a=rs.randn(*shape) * 2 + 0.5, b=rs.randn(*shape) - 0.3, g1=rs.rand(C) + 0.5, b1=rs.randn(C),
                g2=rs.rand(C) + 0.5, b2=rs.randn(C))
    out = {k: nd.array(v.astype('float32'), ctx=ctx) for k, v in arrs.items()}
    for v in out.values():
        v.attach_grad()
    stats = dict(mm1=rs.randn(C) * 0.1, mv1=rs.rand(C) + 0.5, mm2=rs.randn(C) * 0.1, mv2=rs.rand(C) + 0.5)
    out.update({k: nd.array(v.astype('float32'), ctx=ctx) for k, v in stats.items()})
    out['w'] = nd.array(rs.randn(*shape).astype('float32'), ctx=ctx)
    return out


@pytest.mark.parametrize('train', [True, False])
def test_operator_equals_composition_cpu(train):
    """fp32 on the CPU: outputs, all six gradients and both pairs of moving statistics equal
    relu(BatchNorm(a) + BatchNorm(b)) composed from the existing operators, in train and eval mode."""
    ctx = mx.cpu()
    shape = (4, 5, 5, 16)
    kw = dict(axis=3, fix_gamma=False, eps=1e-5, momentum=0.9)
    f = _nd_inputs(ctx, shape, 7)
    r = _nd_inputs(ctx, shape, 7)
    with autograd.record(train_mode=train):
        y = nd.contrib.BatchNormBatchNormAddReLU(f['a'], f['b'], f['g1'], f['b1'], f['g2'], f['b2'], f['mm1'], f['mv1'],
                                                 f['mm2'], f['mv2'], **kw)
        (y * f['w']).sum().backward()
    with autograd.record(train_mode=train):
        sc = nd.BatchNorm(r['b'], r['g2'], r['b2'], r['mm2'], r['mv2'], **kw)
        yr = nd.contrib.BatchNormAddReLU(r['a'], sc, r['g1'], r['b1'], r['mm1'], r['mv1'], **kw)
        (yr * r['w']).sum().backward()
    np.testing.assert_allclose(y.asnumpy(), yr.asnumpy(), rtol=1e-5, atol=1e-5)
    for k in ('a', 'b', 'g1', 'b1', 'g2', 'b2'):
        ref = r[k].grad.asnumpy()
        np.testing.assert_allclose(f[k].grad.asnumpy(), ref, rtol=1e-4, atol=1e-5 * float(np.abs(ref).max() + 1),
                                   err_msg=k)
    for k in ('mm1', 'mv1', 'mm2', 'mv2'):
        np.testing.assert_allclose(f[k].asnumpy(), r[k].asnumpy(), rtol=1e-6, atol=1e-6, err_msg=k)
    if train:
        assert not np.allclose(f['mm2'].asnumpy(), _nd_inputs(ctx, shape, 7)['mm2'].asnumpy())


@pytest.mark.parametrize('name', ['resnet18_v1', 'resnet50_v1b'])
def test_fused_nhwc_resnet_keeps_parameter_names(name, tmp_path):
    """Folding the projection BatchNorm into the tail moves no parameter: the names of collect_params() and of
    save_parameters are those recorded before the operator existed, and a save / load round trip works."""
    with open(GOLDEN) as fh:
        golden = json.load(fh)[name]
    net = gluon.model_zoo.vision.get_model(name, layout='NHWC', fuse=True, classes=10, prefix=name + '_')
    assert list(net.collect_params().keys()) == golden['collect_params']
    assert list(net._collect_params_with_prefix().keys()) == golden['structural']
    net.initialize(mx.init.Xavier())
    x = nd.random.uniform(-1, 1, shape=(2, 32, 32, 3))
    with autograd.record():
        net(x).sum().backward()             # deferred shapes resolved through the folded tails, stats updated
    path = str(tmp_path / 'net.params')
    net.save_parameters(path)
    assert sorted(nd.load(path).keys()) == sorted(golden['structural'])
    net2 = gluon.model_zoo.vision.get_model(name, layout='NHWC', fuse=True, classes=10)
    net2.load_parameters(path)
    np.testing.assert_array_equal(net2(x).asnumpy(), net(x).asnumpy())


# ----------------------------------------------------------------------------- GPU

def _K():
    from mxnet_maintenance_amd.ops import kernels
    assert kernels.available(), 'HIP kernel extension not loaded: %s' % kernels.load_error()
    return kernels


def _bn_ref(x, g, b, eps):
    xf = x.float()
    dims = tuple(range(x.dim() - 1))
    mean = xf.mean(dims)
    var = xf.var(dims, unbiased=False)
    return (xf - mean) / torch.sqrt(var + eps) * g + b, mean, var


# (4,7,7,64): coefficients in registers; (4,5,5,96), (8,3,3,24): per-vector coefficients and spare lanes of the
# reduction geometry; (3,5,5,2048): one channel-block column; (9,64,64,256) fp16: above 4096*256*8 elements, where
# the two-vector main loop and its remainder run
_SHAPES = [(4, 7, 7, 64), (4, 5, 5, 96), (8, 3, 3, 24), (3, 5, 5, 2048)]
_CASES = [(s, d) for s in _SHAPES for d in (torch.float16, torch.bfloat16, torch.float32)]
_CASES.append(((9, 64, 64, 256), torch.float16))


@pytest.mark.gpu
@pytest.mark.parametrize('shape,dtype', _CASES)
def test_dual_tail_matches_fp32_reference(shape, dtype):
    K = _K()
    torch.manual_seed(0)
    dev = 'cuda'
    C, N = shape[-1], shape[0]
    eps, mom = 1e-5, 0.9
    x = (torch.randn(shape, device=dev) * 2 + 0.5).to(dtype)
    z = (torch.randn(shape, device=dev) * 1.5 - 0.3).to(dtype)
    g1, b1 = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
    g2, b2 = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
    dy = torch.randn(shape, device=dev)
    lr = [t.detach().float().requires_grad_() for t in (x, z)] + [t.clone().requires_grad_() for t in (g1, b1, g2, b2)]
    y1, m1, v1 = _bn_ref(lr[0], lr[2], lr[3], eps)
    y2, m2, v2 = _bn_ref(lr[1], lr[4], lr[5], eps)
    # the operator is BatchNorm followed by BatchNormAddReLU in one pass, bit for bit: the normalised shortcut is
    # rounded to the tensors' type before the add (a no-op in fp32), as the addend of the existing add_relu
    # reference is; its gradient passes straight through the rounding
    y2 = y2 + (y2.detach().to(dtype).float() - y2.detach())
    yr = torch.relu(y1 + y2)
    yr.backward(dy)

    lk = [t.detach().requires_grad_() for t in (x, z)] + [t.clone().requires_grad_() for t in (g1, b1, g2, b2)]
    st0 = [torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5,
           torch.randn(C, device=dev) * 0.1, torch.rand(C, device=dev) + 0.5]
    st = [t.clone() for t in st0]
    y, mean, var = K.BatchNormDualTailNHWC.apply(lk[0], lk[1], lk[2], lk[3], lk[4], lk[5], eps, True, st[0], st[1],
                                                 st[2], st[3], mom)
    y.backward(dy.to(dtype))
    tol = {torch.float16: 2e-2, torch.bfloat16: 8e-2, torch.float32: 1e-4}[dtype]
    torch.testing.assert_close(mean, m1, atol=1e-3, rtol=1e-3)
    torch.testing.assert_close(var, v1, atol=1e-3 * v1.abs().max().item(), rtol=1e-3)
    torch.testing.assert_close(y.float(), yr, atol=tol * 4, rtol=tol)
    for i, name in enumerate(('d data', 'd shortcut_data')):
        torch.testing.assert_close(lk[i].grad.float(), lr[i].grad, atol=tol * 4, rtol=tol, msg=lambda m: name + ': ' + m)
    for i, name in ((2, 'd gamma'), (3, 'd beta'), (4, 'd shortcut_gamma'), (5, 'd shortcut_beta')):
        torch.testing.assert_close(lk[i].grad, lr[i].grad, atol=tol * N * 5, rtol=tol, msg=lambda m: name + ': ' + m)
    # moving statistics of both BatchNorms: moving * momentum + batch * (1 - momentum), biased variance
    for got, old, new in zip(st, st0, (m1, v1, m2, v2)):
        want = old * mom + new.detach() * (1 - mom)
        torch.testing.assert_close(got, want, atol=1e-3 * want.abs().max().item(), rtol=1e-3)
    # eval mode: both affines from the moving statistics, one apply launch
    with torch.no_grad():
        ye, _, _ = K.BatchNormDualTailNHWC.apply(x, z, g1, b1, g2, b2, eps, False, st[0], st[1], st[2], st[3], mom)
    ref = torch.relu((x.float() - st[0]) / torch.sqrt(st[1] + eps) * g1 + b1
                     + (z.float() - st[2]) / torch.sqrt(st[3] + eps) * g2 + b2)
    torch.testing.assert_close(ye.float(), ref, atol=tol * 4, rtol=tol)


def _ulp16(v):
    """Spacing of fp16 at |v| (fp32 tensor)."""
    e = torch.frexp(v.abs().clamp_min(2.0 ** -14))[1].float()      # |v| = m * 2^e, m in [0.5, 1)
    return torch.exp2(e - 11)


@pytest.mark.gpu
def test_dual_tail_matches_two_operator_path():
    """Against BatchNorm followed by BatchNormAddReLU (the lazy dy + mask hand-over), fp16, set up as
    test_conv_pw.test_projection_shortcut_lazy_gradient: all six gradients agree within rtol 2e-3, atol 2e-3
    max|ref|. The output may differ by the fp16 rounding of the shortcut that the new path never writes; the tail
    kernel rounds the normalised shortcut as the separate pass stored it, so in fact the outputs are equal."""
    from mxnet_maintenance_amd.ops import hip_ops as H
    from mxnet_maintenance_amd.ops import kernel_fns as KF
    dev = torch.device('cuda', 0)
    torch.manual_seed(5)
    N, Hh, W, C = 4, 14, 14, 256
    x0 = torch.randn(N, Hh, W, C, device=dev).half()
    s0 = torch.randn(N, Hh, W, C, device=dev).half()
    wl = torch.randn(N, Hh, W, C, device=dev)
    names = ('data', 'shortcut_data', 'gamma', 'beta', 'shortcut_gamma', 'shortcut_beta')

    def run(dual, w):
        x = x0.clone().requires_grad_()
        s = s0.clone().requires_grad_()
        torch.manual_seed(9)
        g1 = torch.empty(C, device=dev).uniform_(0.5, 1.5).requires_grad_()
        g2 = torch.empty(C, device=dev).uniform_(0.5, 1.5).requires_grad_()
        b1 = torch.zeros(C, device=dev).requires_grad_()
        b2 = torch.zeros(C, device=dev).requires_grad_()
        rm1, rv1, rm2, rv2 = (torch.zeros(C, device=dev), torch.ones(C, device=dev),
                              torch.zeros(C, device=dev), torch.ones(C, device=dev))
        if dual:
            sc = None
            out = H.batch_norm_dual_add_relu(x, s, g1, b1, g2, b2, rm1, rv1, rm2, rv2, 1e-5, 0.9, False, True, 3)[0]
        else:
            sc = H.batch_norm(s, g2, b2, rm2, rv2, 1e-5, 0.9, False, True, 3, None)[0]
            out = H.batch_norm(x, g1, b1, rm1, rv1, 1e-5, 0.9, False, True, 3, 'relu', addend=sc)[0]
        (out.float() * w).sum().backward()
        return out.detach(), sc, [t.grad.float() for t in (x, s, g1, b1, g2, b2)], (rm1, rv1, rm2, rv2)
    used = KF._DUAL_TAIL_USED[0]
    y_ref, sc_ref, ref, st_ref = run(False, wl)
    assert KF._DUAL_TAIL_USED[0] == used
    y, _, got, st = run(True, wl)
    assert KF._DUAL_TAIL_USED[0] == used + 1
    # the two-operator path rounds the shortcut to fp16 (half a spacing at |sc|) before the add; both outputs are
    # then rounded to fp16 themselves (half a spacing each at the output's magnitude)
    bound = 0.5 * _ulp16(sc_ref.detach().float()) + _ulp16(torch.maximum(y.float().abs(), y_ref.float().abs()))
    excess = ((y.float() - y_ref.float()).abs() - bound).max().item()
    print('output: max |diff| %.3e, max excess over the rounding bound %.3e'
          % ((y.float() - y_ref.float()).abs().max().item(), excess))
    assert excess <= 0
    assert torch.equal(y, y_ref)
    for a, b in zip(st, st_ref):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
    for name, a, b in zip(names, got, ref):
        print('d %s: max |diff| %.3e, max |ref| %.3e' % (name, (a - b).abs().max().item(), b.abs().max().item()))
    for name, a, b in zip(names, got, ref):
        torch.testing.assert_close(a, b, rtol=2e-3, atol=2e-3 * float(b.abs().max() + 1e-6),
                                   msg=lambda m: 'd %s: %s' % (name, m))


@pytest.mark.gpu
def test_resnet50_step_takes_dual_tail_in_projection_blocks():
    """One fused NHWC ResNet-50 training step: the four projection blocks run the folded tail (no separate
    shortcut BatchNorm apply), and every parameter gets a finite, non-zero gradient."""
    from mxnet_maintenance_amd.ops import kernel_fns as KF
    ctx = mx.gpu(0)
    mx.random.seed(3)
    net = gluon.model_zoo.vision.get_model('resnet50_v1b', layout='NHWC', fuse=True, classes=10)
    net.initialize(mx.init.Xavier(), ctx=ctx)
    net.cast('float16')
    net.hybridize(static_alloc=True, static_shape=True)
    x = nd.random.uniform(-1, 1, shape=(8, 64, 64, 3), ctx=ctx).astype('float16')
    y = nd.array([1, 2, 3, 4, 5, 6, 7, 8], ctx=ctx)
    loss_fn = gluon.loss.SoftmaxCrossEntropyLoss()
    used = KF._DUAL_TAIL_USED[0]
    with autograd.record():
        loss = loss_fn(net(x), y)
    loss.backward()
    # each folded tail replaces one separate shortcut BatchNorm apply launch
    assert KF._DUAL_TAIL_USED[0] == used + 4
    grads = [p.grad(ctx).astype('float32').asnumpy() for p in net.collect_params().values() if p.grad_req != 'null']
    assert all(np.isfinite(g).all() for g in grads)
    assert sum(float(np.abs(g).sum()) > 0 for g in grads) == len(grads)
    assert np.isfinite(loss.asnumpy()).all()


@pytest.mark.gpu
def test_dual_tail_direct_grad_accumulate_and_null():
    """Inside mx.autograd.backward all four gamma / beta gradients are added straight into the leaves' fp32 .grad
    buffers (what grad_req 'add' and the zeroed 'write' buffers rely on) and the leaves' hooks still fire; a
    parameter that takes no gradient (grad_req 'null') gets none and leaves the others unchanged."""
    from mxnet_maintenance_amd import _state
    K = _K()
    torch.manual_seed(2)
    dev = 'cuda'
    shape = (4, 9, 9, 128)
    C = shape[-1]
    x = torch.randn(shape, device=dev).half()
    z = torch.randn(shape, device=dev).half()
    dy = torch.randn(shape, device=dev).half()
    p0 = [torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev), torch.rand(C, device=dev) + 0.5,
          torch.randn(C, device=dev)]

    def run(direct, frozen=()):
        ps = [t.clone().requires_grad_(i not in frozen) for i, t in enumerate(p0)]
        fired = []
        for i, t in enumerate(ps):
            if i not in frozen:
                t.grad = torch.full((C,), 0.25, device=dev)
                t.register_post_accumulate_grad_hook(lambda _t, i=i: fired.append(i))
        xk, zk = x.clone().requires_grad_(), z.clone().requires_grad_()
        _state.DIRECT_GRAD[0] += int(direct)
        try:
            y, _, _ = K.BatchNormDualTailNHWC.apply(xk, zk, ps[0], ps[1], ps[2], ps[3], 1e-5, True,
                                                    torch.zeros(C, device=dev), torch.ones(C, device=dev),
                                                    torch.zeros(C, device=dev), torch.ones(C, device=dev), 0.9)
            torch.autograd.backward(y, dy)
        finally:
            _state.DIRECT_GRAD[0] -= int(direct)
        return [None if t.grad is None else t.grad.clone() for t in ps], xk.grad.clone(), zk.grad.clone(), sorted(fired)
    gd, xd, zd, fd = run(True)
    gr, xr, zr, fr = run(False)
    for a, b in zip(gd, gr):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(xd, xr)
    torch.testing.assert_close(zd, zr)
    assert fd == [0, 1, 2, 3] and fr == [0, 1, 2, 3]
    # shortcut gamma and main beta frozen
    for direct in (True, False):
        gn, xn, zn, fn = run(direct, frozen=(1, 2))
        assert gn[1] is None and gn[2] is None and fn == [0, 3]
        torch.testing.assert_close(gn[0], gr[0], rtol=1e-4, atol=1e-3)
        torch.testing.assert_close(gn[3], gr[3], rtol=1e-4, atol=1e-3)
        torch.testing.assert_close(xn, xr)
        torch.testing.assert_close(zn, zr)
