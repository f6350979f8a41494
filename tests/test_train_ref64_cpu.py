"""The float64 restatements of the update step's kernels (tests/_train_ref64.py) checked without a GPU:
against torch's own float64 ops on NCHW data, the fp32 operation-for-operation BatchNorm restatements
against the float64 formulas, the preconditions of every integer case the GPU file demands bit for
bit, and the statistics bound against an fp32 emulation of the kernels' summation order (the bound can
be met by the algorithm as designed) and against the unshifted E[x^2] - E[x]^2 (the bound has teeth)."""
import pytest
import torch
import torch.nn.functional as F

from tests import _train_ref64 as R


def _nchw(t):  # [n,64,C] -> [n,C,8,8]
    return t.permute(0, 2, 1).reshape(t.shape[0], t.shape[2], 8, 8)


def _nhwc(t):  # [n,C,8,8] -> [n,64,C]
    return t.reshape(t.shape[0], t.shape[1], 64).permute(0, 2, 1).contiguous()


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("n,ci_real,ci,co", [(2, 5, 8, 7), (3, 12, 16, 16)])
def test_conv_restatements_equal_torch_float64(n, ci_real, ci, co):
    g = torch.Generator().manual_seed(n + co)
    x = torch.zeros(n, 64, ci, dtype=torch.float16)
    x[..., :ci_real] = torch.randn(n, 64, ci_real, generator=g).half()
    w = torch.randn(co, ci_real, 3, 3, generator=g).half()
    b = torch.randn(co, generator=g)
    dy = torch.randn(n, 64, co, generator=g).half()
    x64, w64, dy64 = _nchw(x[..., :ci_real].double()), w.double(), _nchw(dy.double())
    assert _rel(R.conv_fwd(x, w, b), _nhwc(F.conv2d(x64, w64, b.double(), padding=1))) < 1e-12
    assert _rel(R.conv_dgrad(dy, w), _nhwc(torch.nn.grad.conv2d_input(x64.shape, w64, dy64, padding=1))) < 1e-12
    assert _rel(R.conv_wgrad(dy, x, ci_real), torch.nn.grad.conv2d_weight(x64, w64.shape, dy64, padding=1)) < 1e-12
    # the abs variants bound their own sums and are the same sums of the absolute values
    assert bool((R.conv_fwd(x, w, b).abs() <= R.conv_fwd_abs(x, w, b) * (1 + 1e-12)).all())
    assert _rel(R.conv_dgrad_abs(dy, w), R.conv_dgrad(dy.abs(), w.abs())) < 1e-12
    assert _rel(R.conv_wgrad_abs(dy, x, ci_real), R.conv_wgrad(dy.abs(), x.abs(), ci_real)) < 1e-12
    # layout helpers against direct indexing
    wf, wt = R.weight_images(w.float(), ci)
    for o, c, t in [(0, 0, 0), (co - 1, ci_real - 1, 8), (1, 2, 5), (co // 2, 1, 3)]:
        assert wf[o, t, c] == w[o, c, t // 3, t % 3] and wt[c, 8 - t, o] == w[o, c, t // 3, t % 3]
    assert not bool(wf[:, :, ci_real:].any()) and not bool(wt[ci_real:].any())
    planes = torch.randn(n, 12, 8, 8, generator=g)
    p = R.planes_nhwc(planes, 64)
    assert torch.equal(p[..., :12], _nhwc(planes).half()) and not bool(p[..., 12:].any())


@pytest.mark.parametrize("n,C,res,relu", [(2, 64, False, True), (3, 128, True, False)])
def test_bn_restatements_equal_torch_float64(n, C, res, relu):
    g = torch.Generator().manual_seed(n * C)
    x = (torch.randn(n, 64, C, generator=g) * 2 + 0.5).half()
    r = torch.randn(n, 64, C, generator=g).half() if res else None
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    dy = torch.randn(n, 64, C, generator=g).half()
    eps = 1e-5
    mean, var, invstd = R.bn_stats(x, eps)
    xa = _nchw(x.double()).requires_grad_(True)
    ga, ba = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    bn = F.batch_norm(xa, None, None, ga, ba, training=True, eps=R.eps32(eps))
    y = bn + _nchw(r.double()) if res else bn
    y = torch.relu(y) if relu else y
    bn64, y64 = R.bn_apply64(x, mean, invstd, gamma, beta, r, relu)
    assert _rel(bn64, _nhwc(bn.detach())) < 1e-12 and _rel(y64, _nhwc(y.detach())) < 1e-12
    assert _rel(var, x.double().reshape(-1, C).var(0, unbiased=False)) < 1e-12
    y.backward(_nchw(dy.double()))
    y16 = y64.half()  # the mask's source: y > 0 survives the rounding or the value is 0 either way
    dx, dres, dgamma, dbeta = R.bn_backward64(x, dy, y16, relu, mean, invstd, gamma)
    assert _rel(dx, _nhwc(xa.grad)) < 1e-12
    assert _rel(dgamma, ga.grad) < 1e-12 and _rel(dbeta, ba.grad) < 1e-12

    # the fp32 operation-for-operation restatements lie within fp16 rounding of the float64 formulas
    m32, iv32 = mean.float(), invstd.float()
    y32 = R.bn_apply32(x, m32, iv32, gamma, beta, r, relu)
    mag = bn64.abs() + (r.double().abs() if res else 0.0)  # two roundings with a residual, each 2^-11 of its value
    tol = (2.0 ** -10 if res else 2.0 ** -11) * mag * (1 + 2.0 ** -8) + 2.0 ** -24
    assert bool(((y32.double() - y64).abs() <= tol).all())
    sg, sgx, _, _ = R.bn_sums64(x, dy, y32, relu, m32, iv32)
    dx64 = R.bn_backward64(x, dy, y32, relu, m32, iv32, gamma)[0]
    dx32, dres32 = R.bn_backward32(x, dy, y32, relu, m32, iv32, gamma, sg.float(), sgx.float())
    rows = n * 64
    xh = ((x.double() - m32.double()) * iv32.double()).abs()
    mag = (gamma.double() * iv32.double()).abs() * (dy.double().abs() + sg.abs() / rows + xh * sgx.abs() / rows)
    assert bool(((dx32.double() - dx64).abs() <= 2.0 ** -11 * dx64.abs() + 2.0 ** -20 * mag + 2.0 ** -24).all())
    assert torch.equal(dres32, R._masked(dy, y32, relu))


def test_head_restatements_equal_torch_float64():
    g = torch.Generator().manual_seed(9)
    h = torch.randn(2, 64, 512, generator=g).half()
    w, b = torch.randn(3, 512, generator=g).half(), torch.randn(3, generator=g)
    dout = torch.randn(2, 64, 4, generator=g).half()
    ha, wa, ba = (t.double().requires_grad_(True) for t in (h, w, b))
    out = F.conv2d(_nchw(ha), wa.reshape(3, 512, 1, 1), ba)
    assert _rel(R.head_fwd(h, w, b), _nhwc(out.detach())) < 1e-12
    out.backward(_nchw(dout[..., :3].double()))
    dh, dw, db = R.head_bwd(h, dout, w)
    assert _rel(dh, ha.grad) < 1e-12 and _rel(dw, wa.grad) < 1e-12 and _rel(db, ba.grad) < 1e-12


@pytest.mark.parametrize("kind,shape", [("conv", s) for s in R.CONV_INT_CASES] + [("dgrad", s) for s in R.DGRAD_INT_CASES]
                         + [("wgrad", s) for s, _ in R.WGRAD_INT_CASES] + [("head", (n,)) for n in R.HEAD_INT_CASES])
def test_int_case_preconditions(kind, shape):
    """int_case asserts them itself (sum |terms| < 2^24, finite in fp16, one rounding); here also that the
    cases are not trivial: the outputs are neither all zero nor all fp16-exact small integers only."""
    c = R.int_case(kind, *shape)
    outs = {"conv": ("y16", "ya16"), "dgrad": ("dx16", "dxa16"), "wgrad": ("dw32",),
            "head": ("out16", "dh16", "dw32", "db32")}[kind]
    for name in outs:
        t = getattr(c, name)
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0, name
        assert torch.equal(t.float(), t.float().half().float()), name
    print(f"{kind} {shape}: " + ", ".join(f"max |{k}| {float(getattr(c, k).abs().max()):.0f}" for k in outs))


@pytest.mark.parametrize("n,C,mean,std", R.BN_STATS_CASES)
def test_stats_emulation_is_inside_the_bound(n, C, mean, std):
    """The kernels' summation order in fp32 (row lanes, 256-row blocks, float64 combine, k = row 0) stays
    inside the statistics bound on every case of the GPU file; the same order without the shift (k = 0)
    breaks the variance bound on the two large-mean cases."""
    eps = 1e-5
    x = R.bn_case(n, C, mean, std)
    b = R.bn_stats_bounds(x, eps)
    rm, rv, ri = R.bn_stats_ratios(b, *R.bn_stats_emul32(x, eps), eps)
    print(f"BN stats ({n}, {C}, {mean}, {std}) emulation error / bound: mean {rm:.3f}, var {rv:.3f}, invstd {ri:.3f}; "
          f"max |delta| {float(b.delta.abs().max()):.2f}")
    assert rm <= 1 and rv <= 1 and ri <= 1
    if (n, C) == (7, 128):
        assert float(b.var[R.BN_CONST_CH]) == 0 and 9.5 < float(b.delta[R.BN_FAR_CH]) < 10.5
    nm, nv, _ = R.bn_stats_ratios(b, *R.bn_stats_emul32(x, eps, shift=False), eps)
    print(f"    without the shift: mean {nm:.3g}, var {nv:.3g}")
    if (n, C, mean, std) in R.BN_LARGE_MEAN_CASES:
        assert nv > 1, "the unshifted E[x^2] - E[x]^2 passes the variance bound: the bound has no teeth"
