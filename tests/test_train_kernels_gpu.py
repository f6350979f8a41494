"""The update step's HIP kernels (csrc/kv_train.hip) at their edges, against the float64 restatements of
tests/_train_ref64.py (checked on the CPU by test_train_ref64_cpu.py):

* convolution forward, data gradient, weight gradient and the 1x1 heads on integer-valued inputs, where
  every product and partial sum is an integer below 2^24: fp32 accumulation in any order is exact, the one
  fp16 rounding is unambiguous, so the kernel's bits must be the reference's. The shapes are the smallest
  that reach each branch of the grid mappings and pipelines (one stage, odd stage counts, one and eight
  channel blocks, idle workgroups, board tails, every split-count class of the weight gradient, empty splits);
* the same kernels on Gaussian data inside the worst-case fp32 accumulation bound of _train_ref64.accum_bound;
* the BatchNorm statistics inside the shifted-sum bound (it carries the delta^2 = ((x[0] - mean) / std)^2
  term), the elementwise kernels bit for bit against fp32 operation-for-operation restatements, the
  reductions inside their summation bound -- the dx channel sums (exact value 0) in absolute terms against
  the float64 sum of the kernel's own fp16 dx;
* the layout kernels bit for bit.

Worst error-to-bound ratios measured on an MI355X (printed by the tests, -s shows them):
  convolutions, Gaussian (9, 256, 512): forward 0.201, data gradient 0.077, weight gradient 0.613;
      weight gradient (33, 64, 64, 64) 0.184
  heads, Gaussian n = 5: forward 0.474, dh 0.996 (3 terms: the bound is the fp16 rounding itself), dw 0.611, db 0.580
  statistics (mean / var / invstd), the CPU emulation of the kernels' order gives the same figures:
      (1, 64, 0.5, 2) 0.028 / 0.364 / 0.501     (7, 128, 0.5, 2) 0.071 / 0.203 / 0.562 (max |delta| 9.92)
      (5, 320, 0.5, 2) 0.052 / 0.239 / 0.555    (5, 448, 0.5, 2) 0.078 / 0.219 / 0.581
      (3, 512, 1000, 4) 0.166 / 0.056 / 0.588   (257, 64, 100, 0.5) 0.297 / 0.061 / 0.524
  BN sums (dbeta / dgamma / channel sum / dx sum): (257, 64) 0.001 / 0.003 / 0.000 / 0.001,
      (5, 448) 0.004 / 0.011 / 0.003 / 0.006 (a worst-case bound: random rounding errors stay far inside it; a
      dropped block partial is one part in 65 or 257 of sum |terms| and misses it by orders of magnitude)"""
import ctypes

import pytest
import torch

from knightvision_amd import _lib
from knightvision_amd import train_ops as TO
from tests import _train_ref64 as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A  # fp16 203.25: no integer case produces it


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(got, want, what, zero_sign=True):
    """zero_sign=False: -0 and +0 count as the same value (every other bit pattern still has to match). Only
    for a sum that does not start from +0, where (-0) + (-0) = -0 is the correct IEEE result of the kernel's
    own operations and the float64 reference, normalised to +0, cannot know it."""
    g, w = _bits(got), _bits(want)
    if not zero_sign:
        neg0 = -0x8000 if g.dtype == torch.int16 else -0x80000000
        g, w = torch.where(g == neg0, torch.zeros_like(g), g), torch.where(w == neg0, torch.zeros_like(w), w)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ, first at {i}: "
                             f"got {float(got.detach().cpu()[i])!r}, want {float(want.detach().cpu()[i])!r}")


def _conv_guarded(x, w_img, bias, add, n, co):
    """kv_tr_conv3x3_add_f16 into a buffer of n + 8 boards prefilled with SENTINEL; returns the whole buffer."""
    y = torch.full(((n + 8) * 64 * co,), SENTINEL, dtype=torch.int16, device=x.device).view(torch.float16)
    y = y.view(n + 8, 64, co)
    _lib.check(_lib.lib().kv_tr_conv3x3_add_f16(x.data_ptr(), n, x.shape[2], w_img.data_ptr(), TO._ptr(bias), co,
                                                TO._ptr(add), y.data_ptr(), TO._stream(x)), "kv_tr_conv3x3_add_f16")
    return y


def _check_guarded(y, n, want, what):
    assert bool((_bits(y[n:]) == SENTINEL).all()), f"{what}: boards past n were written"
    _same_bits(y[:n], want, what)


# ------------------------------------------------- a. convolution, exact --
@pytest.mark.parametrize("n,ci,co", R.CONV_INT_CASES)
def test_conv_forward_bit_for_bit(n, ci, co):
    c = R.int_case("conv", n, ci, co)
    wf, _ = TO.conv_weight_images(c.w32.cuda(), ci, False)
    _same_bits(wf, R.weight_images(c.w32, ci)[0], "forward weight image")
    x, bias, add = c.x16.cuda(), c.bias32.cuda(), c.add16.cuda()
    _check_guarded(_conv_guarded(x, wf, bias, None, n, co), n, c.y16, "forward")
    _check_guarded(_conv_guarded(x, wf, bias, add, n, co), n, c.ya16, "forward + fused add")
    _same_bits(TO.conv3x3_f16(x, wf, bias, add), c.ya16, "forward + fused add (wrapper)")


@pytest.mark.parametrize("n,ci,co", R.DGRAD_INT_CASES)
def test_conv_data_gradient_bit_for_bit(n, ci, co):
    c = R.int_case("dgrad", n, ci, co)
    _, wt = TO.conv_weight_images(c.w32.cuda(), ci, True)
    _same_bits(wt, R.weight_images(c.w32, ci)[1], "flipped weight image")
    dy, add = c.dy16.cuda(), c.add16.cuda()
    _check_guarded(_conv_guarded(dy, wt, None, None, n, ci), n, c.dx16, "data gradient")
    _check_guarded(_conv_guarded(dy, wt, None, add, n, ci), n, c.dxa16, "data gradient + fused add")


# ------------------------------------------------ b. weight gradient, exact --
@pytest.mark.parametrize("shape,splits", R.WGRAD_INT_CASES)
def test_wgrad_bit_for_bit(shape, splits):
    n, ci_real, ci, co = shape
    s = ctypes.c_int(0)
    nbytes = _lib.lib().kv_tr_wgrad_workspace(n, ci, co, ctypes.byref(s))
    assert s.value == splits, f"{shape}: {s.value} splits, this case is here for {splits}"
    assert nbytes == splits * co * 9 * ci * 4
    c = R.int_case("wgrad", n, ci_real, ci, co)
    dy, x = c.dy16.cuda(), c.x16.cuda()
    a = TO.conv3x3_wgrad_f16(dy, x, ci_real)
    b = TO.conv3x3_wgrad_f16(dy, x, ci_real)
    assert a.shape == (co, ci_real, 3, 3)
    assert torch.equal(a.cpu(), a.cpu().half().float()), "weight gradient not fp16-representable"
    _same_bits(a, b, "two calls")
    _same_bits(a, c.dw32, "weight gradient")


# --------------------------------------------------- c. real-valued data --
def _ratio(got, ref64, abs64, k):
    return float(((got.detach().cpu().double() - ref64).abs() / R.accum_bound(ref64, abs64, k)).max())


def test_conv_gaussian_within_accumulation_bound():
    n, ci, co = 9, 256, 512
    g = torch.Generator().manual_seed(2024)
    x = torch.randn(n, 64, ci, generator=g).half()
    w = torch.randn(co, ci, 3, 3, generator=g) / (3.0 * ci ** 0.5)
    b = (torch.randn(co, generator=g) * 0.1).half().float()
    dy = torch.randn(n, 64, co, generator=g).half()
    w16 = w.half()
    xc, dyc = x.cuda(), dy.cuda()
    wf, wt = TO.conv_weight_images(w.cuda(), ci, True)
    r = {"forward": _ratio(TO.conv3x3_f16(xc, wf, b.cuda()), R.conv_fwd(x, w16, b), R.conv_fwd_abs(x, w16, b),
                           9 * ci + 1),
         "data gradient": _ratio(TO.conv3x3_f16(dyc, wt, None), R.conv_dgrad(dy, w16), R.conv_dgrad_abs(dy, w16),
                                 9 * co),
         "weight gradient": _ratio(TO.conv3x3_wgrad_f16(dyc, xc, ci), R.conv_wgrad(dy, x, ci),
                                   R.conv_wgrad_abs(dy, x, ci), n * 64)}
    print(f"conv ({n}, {ci}, {co}) worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1 for v in r.values()), r


def test_wgrad_gaussian_16_splits_within_accumulation_bound():
    n, ci, co = 33, 64, 64
    g = torch.Generator().manual_seed(33)
    x, dy = torch.randn(n, 64, ci, generator=g).half(), torch.randn(n, 64, co, generator=g).half()
    r = _ratio(TO.conv3x3_wgrad_f16(dy.cuda(), x.cuda(), ci), R.conv_wgrad(dy, x, ci), R.conv_wgrad_abs(dy, x, ci),
               n * 64)
    print(f"wgrad ({n}, {ci}, {ci}, {co}) worst error / bound: {r:.3f}")
    assert r <= 1


def _bn_stats(xc, eps):
    n, _, C = xc.shape
    L = _lib.lib()
    ws = TO._workspace(xc.device, L.kv_tr_bn_workspace(n * 64, C))
    mean = torch.empty(C, dtype=torch.float32, device=xc.device)
    var, invstd = torch.empty_like(mean), torch.empty_like(mean)
    _lib.check(L.kv_tr_bn_stats_f16(xc.data_ptr(), n * 64, C, float(eps), mean.data_ptr(), var.data_ptr(),
                                    invstd.data_ptr(), ws.data_ptr(), ws.numel(), TO._stream(xc)), "kv_tr_bn_stats_f16")
    return mean, var, invstd


def _bn_apply(xc, mean, invstd, gamma, beta, res, relu):
    n, _, C = xc.shape
    y = torch.empty_like(xc)
    _lib.check(_lib.lib().kv_tr_bn_apply_f16(xc.data_ptr(), n * 64, C, mean.data_ptr(), invstd.data_ptr(),
                                             gamma.data_ptr(), beta.data_ptr(), TO._ptr(res), int(relu), y.data_ptr(),
                                             TO._stream(xc)), "kv_tr_bn_apply_f16")
    return y


def _bn_backward(xc, dyc, yc, relu, mean, invstd, gamma):
    """(dx, dres, dgamma, dbeta, dxsum) of kv_tr_bn_backward_f16."""
    n, _, C = xc.shape
    L = _lib.lib()
    ws = TO._workspace(xc.device, L.kv_tr_bn_workspace(n * 64, C))
    dx, dres = torch.empty_like(xc), torch.empty_like(xc)
    dgamma = torch.empty(C, dtype=torch.float32, device=xc.device)
    dbeta, dxsum = torch.empty_like(dgamma), torch.empty_like(dgamma)
    _lib.check(L.kv_tr_bn_backward_f16(xc.data_ptr(), dyc.data_ptr(), TO._ptr(yc), n * 64, C, int(relu),
                                       mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), dgamma.data_ptr(),
                                       dbeta.data_ptr(), dx.data_ptr(), dres.data_ptr(), dxsum.data_ptr(),
                                       ws.data_ptr(), ws.numel(), TO._stream(xc)), "kv_tr_bn_backward_f16")
    return dx, dres, dgamma, dbeta, dxsum


@pytest.mark.parametrize("n,C,mean,std", R.BN_STATS_CASES)
def test_bn_statistics_within_shifted_sum_bound(n, C, mean, std):
    eps = 1e-5
    x = R.bn_case(n, C, mean, std)
    b = R.bn_stats_bounds(x, eps)
    m, v, iv = _bn_stats(x.cuda(), eps)
    rm, rv, ri = R.bn_stats_ratios(b, m, v, iv, eps)
    print(f"BN stats ({n}, {C}, {mean}, {std}) error / bound: mean {rm:.3f}, var {rv:.3f}, invstd {ri:.3f}; "
          f"max |delta| {float(b.delta.abs().max()):.2f}")
    assert rm <= 1 and rv <= 1 and ri <= 1
    if (n, C) == (7, 128):
        assert float(v[R.BN_CONST_CH]) <= 2.0 ** -24 * 0.71875 ** 2
        assert abs(float(iv[R.BN_CONST_CH]) * (float(v[R.BN_CONST_CH]) + R.eps32(eps)) ** 0.5 - 1) <= 2.0 ** -23


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("C", [64, 320, 512])
def test_bn_elementwise_bit_for_bit(n, C):
    """bn_apply_kernel (res x relu) and bn_backward_kernel's dx / dres (relu 0, 1) against the fp32
    operation-for-operation restatements, fed the kernel's own mean, invstd, dbeta and dgamma."""
    g = torch.Generator().manual_seed(n * 1000 + C)
    x = (torch.randn(n, 64, C, generator=g) * 2 + 0.5).half()
    res = torch.randn(n, 64, C, generator=g).half()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    dy = torch.randn(n, 64, C, generator=g).half()
    xc, rc, gc, bc, dyc = (t.cuda() for t in (x, res, gamma, beta, dy))
    mean, _, invstd = _bn_stats(xc, 1e-5)
    ys = {}
    for has_res in (False, True):
        for relu in (False, True):
            y = _bn_apply(xc, mean, invstd, gc, bc, rc if has_res else None, relu)
            _same_bits(y, R.bn_apply32(x, mean, invstd, gamma, beta, res if has_res else None, relu),
                       f"bn_apply res={has_res} relu={relu}")
            ys[has_res, relu] = y
    for relu in (False, True):
        yc = ys[True, relu]
        dx, dres, dgamma, dbeta, _ = _bn_backward(xc, dyc, yc if relu else None, relu, mean, invstd, gc)
        want_dx, want_dres = R.bn_backward32(x, dy, yc, relu, mean, invstd, gamma, dbeta, dgamma)
        _same_bits(dres, want_dres, f"bn_backward dres relu={relu}")
        _same_bits(dx, want_dx, f"bn_backward dx relu={relu}")


@pytest.mark.parametrize("n,C", [(257, 64), (5, 448)])
def test_bn_sums_within_summation_bound(n, C):
    """dbeta, dgamma, the channel sums and the fused dx sums: (257, 64) has 65 statistics blocks (more than the
    finalize kernel's 64 groups) and 257 dx blocks."""
    g = torch.Generator().manual_seed(n + C)
    x = (torch.randn(n, 64, C, generator=g) * 2 + 0.5).half()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    dy = torch.randn(n, 64, C, generator=g).half()
    xc, gc, bc, dyc = (t.cuda() for t in (x, gamma, beta, dy))
    mean, _, invstd = _bn_stats(xc, 1e-5)
    yc = _bn_apply(xc, mean, invstd, gc, bc, None, True)
    dx, _, dgamma, dbeta, dxsum = _bn_backward(xc, dyc, yc, True, mean, invstd, gc)
    sg, sgx, asg, asgx = R.bn_sums64(x, dy, yc, True, mean, invstd)
    err = lambda got, ref: (got.cpu().double() - ref).abs()
    r = {"dbeta": float((err(dbeta, sg) / R.bn_sum_bound(sg, asg, C)).max()),
         "dgamma": float((err(dgamma, sgx) / R.bn_sum_bound(sgx, asgx, C)).max())}
    cs, acs = dy.double().sum(dim=(0, 1)), dy.double().abs().sum(dim=(0, 1))
    r["channel sum"] = float((err(TO.channel_sum_f16(dyc), cs) / R.bn_sum_bound(cs, acs, C)).max())
    # the dx sums' true value is 0: the kernel's own fp16 dx summed in float64 is what it must reproduce,
    # in absolute terms
    ds, ads = dx.cpu().double().sum(dim=(0, 1)), dx.cpu().double().abs().sum(dim=(0, 1))
    r["dx sum"] = float((err(dxsum, ds) / R.bn_sum_bound(ds, ads, C, block_rows=64)).max())
    print(f"BN sums ({n}, {C}) worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) +
          f"; max |dx sum| {float(ds.abs().max()):.3e} of sum |dx| {float(ads.max()):.3e}")
    assert all(v <= 1 for v in r.values()), r


# ------------------------------------------------------------- 1x1 heads --
def _head_fwd(h, w16, b32):
    n = h.shape[0]
    out = torch.full((n * 64 * 4,), SENTINEL, dtype=torch.int16, device=h.device).view(torch.float16).view(n, 64, 4)
    _lib.check(_lib.lib().kv_tr_head1x1_f16(h.data_ptr(), n * 64, w16.data_ptr(), b32.data_ptr(), out.data_ptr(),
                                            TO._stream(h)), "kv_tr_head1x1_f16")
    return out


def _head_bwd(h, dout, w16):
    n = h.shape[0]
    L = _lib.lib()
    ws = TO._workspace(h.device, L.kv_tr_head1x1_workspace(n * 64))
    dh = torch.empty_like(h)
    dw = torch.empty((3, 512), dtype=torch.float32, device=h.device)
    db = torch.empty(3, dtype=torch.float32, device=h.device)
    _lib.check(L.kv_tr_head1x1_backward_f16(h.data_ptr(), dout.data_ptr(), n * 64, w16.data_ptr(), dh.data_ptr(),
                                            dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), TO._stream(h)),
               "kv_tr_head1x1_backward_f16")
    return dh, dw, db


@pytest.mark.parametrize("n", R.HEAD_INT_CASES)
def test_heads_bit_for_bit(n):
    """n = 17: 5 block partials (the reduce kernel's strided loop); n = 129: 8,256 rows, more than the forward's
    2,048 workgroups x 4 rows. dout's column 3 is non-zero and must not reach any output."""
    c = R.int_case("head", n)
    h, w16, b32, dout = c.h16.cuda(), c.w16.cuda(), c.b32.cuda(), c.dout16.cuda()
    out = _head_fwd(h, w16, b32)
    assert bool((_bits(out[..., 3]) == SENTINEL).all()), "the forward wrote column 3"
    _same_bits(out[..., :3], c.out16, "head forward")
    dh, dw, db = _head_bwd(h, dout, w16)
    # dh = fp16(d0 w0 + d1 w1 + d2 w2) has no +0 to start from: three products of -0 give -0
    _same_bits(dh, c.dh16, "head data gradient", zero_sign=False)
    _same_bits(dw, c.dw32, "head weight gradient")
    _same_bits(db, c.db32, "head bias gradient")


def test_heads_gaussian_within_accumulation_bound():
    n = 5
    g = torch.Generator().manual_seed(55)
    h = torch.randn(n, 64, 512, generator=g).half()
    w16 = (torch.randn(3, 512, generator=g) / 20).half()
    b32 = (torch.randn(3, generator=g) * 0.1).half().float()
    dout = torch.randn(n, 64, 4, generator=g).half()
    hc, wc = h.cuda(), w16.cuda()
    out = _head_fwd(hc, wc, b32.cuda())
    dh, dw, db = _head_bwd(hc, dout.cuda(), wc)
    ref, ab = R.head_bwd(h, dout, w16), R.head_bwd_abs(h, dout, w16)
    r = {"forward": _ratio(out[..., :3], R.head_fwd(h, w16, b32), R.head_fwd_abs(h, w16, b32), 513),
         "dh": _ratio(dh, ref[0], ab[0], 3), "dw": _ratio(dw, ref[1], ab[1], n * 64),
         "db": _ratio(db, ref[2], ab[2], n * 64)}
    print(f"heads n = {n} worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1 for v in r.values()), r


# --------------------------------------------------------- layout kernels --
@pytest.mark.parametrize("n", [1, 3])
def test_planes_to_nhwc_bit_for_bit(n):
    planes = torch.randn(n, 12, 8, 8, generator=torch.Generator().manual_seed(n))
    _same_bits(TO.planes_to_nhwc(planes.cuda(), 64), R.planes_nhwc(planes, 64), "planes_to_nhwc")


@pytest.mark.parametrize("co,ci_real,ci", [(256, 12, 64), (128, 128, 128)])
def test_conv_weight_images_bit_for_bit(co, ci_real, ci):
    w = torch.randn(co, ci_real, 3, 3, generator=torch.Generator().manual_seed(co + ci))
    wf, wt = TO.conv_weight_images(w.cuda(), ci, True)
    want_f, want_t = R.weight_images(w, ci)
    _same_bits(wf, want_f, "forward image")
    _same_bits(wt, want_t, "flipped image")
