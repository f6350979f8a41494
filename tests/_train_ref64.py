"""Plain float64 restatements of the update step's kernels
(knightvision_amd/csrc/kv_train.hip), in the kernels' own layouts: activations
NHWC [n, 64 squares, C], convolution weights [co, ci_real, 3, 3], everything
computed in float64 from the fp16 / fp32 *values* the kernel receives. CPU,
torch only. Also here, because the CPU and the GPU tests share them:

* integer-valued cases (`int_case`) on which every product and partial sum of
  the convolutions and the 1x1 heads is an integer below 2^24, so fp32
  accumulation in any order is exact and the kernel's fp16 result is defined
  bit for bit. `int_case` asserts those preconditions itself;
* fp32 operation-for-operation restatements of the BatchNorm elementwise
  kernels (`bn_apply32`, `bn_backward32`), which run under `fp contract(off)`:
  separate torch ops on the CPU round as the kernel's separate instructions do;
* an fp32 emulation of the statistics kernels' summation order
  (`bn_stats_emul32`) and the statistics bound (`bn_stats_bounds`) that both
  it and the GPU kernel are held to.

Shared by tests/test_train_ref64_cpu.py and tests/test_train_kernels_gpu.py;
not a test module itself."""
import functools
import types

import torch

F16_MAX = 65504.0
TAPS = [(t // 3 - 1, t % 3 - 1) for t in range(9)]  # tap t = kh * 3 + kw reads square p + (kh - 1) * 8 + (kw - 1)

# ------------------------------------------------------------------ cases --
# convolution forward (n, ci, co), section "a" of the GPU file
CONV_INT_CASES = [(1, 16, 128), (8, 32, 128), (9, 48, 256), (17, 64, 512), (9, 64, 1024), (3, 512, 512)]
# data gradient, in the forward's (n, ci, co): the kernel runs on dy [n, 64, co] with the flipped image
# [ci, 9, co], so its own input depth is co (a multiple of 16) and its output width ci (a multiple of 128)
DGRAD_INT_CASES = [(9, 128, 256), (3, 512, 512), (17, 128, 64), (1, 128, 16)]
# weight gradient (n, ci_real, ci, co) -> the split count kv_tr_wgrad_workspace must give
WGRAD_INT_CASES = [((1, 64, 64, 64), 1), ((3, 64, 64, 64), 2), ((5, 192, 192, 64), 2), ((7, 128, 128, 192), 4),
                   ((16, 64, 64, 64), 8), ((17, 64, 64, 64), 8), ((33, 64, 64, 64), 16), ((130, 12, 64, 256), 64),
                   # beyond 8 splits the cases above leave the last splits empty: here the last of 16 owns boards
                   ((32, 64, 64, 64), 16)]
HEAD_INT_CASES = [1, 6, 17, 129]
# BatchNorm statistics (n, C, mean, std)
BN_STATS_CASES = [(1, 64, 0.5, 2.0), (7, 128, 0.5, 2.0), (5, 320, 0.5, 2.0), (5, 448, 0.5, 2.0),
                  (3, 512, 1000.0, 4.0), (257, 64, 100.0, 0.5)]
BN_LARGE_MEAN_CASES = [(3, 512, 1000.0, 4.0), (257, 64, 100.0, 0.5)]
BN_CONST_CH, BN_FAR_CH = 5, 77  # the two special channels of the (7, 128) case


def _d(t):
    return t.detach().to("cpu", torch.float64)


# ----------------------------------------------------------- convolutions --
def _shift(x, dr, dc):
    """s[n, p, c] = x[n, p + dr * 8 + dc, c] where that square is on the 8x8 board, else 0."""
    n, _, c = x.shape
    xp = torch.zeros(n, 10, 10, c, dtype=x.dtype)
    xp[:, 1:9, 1:9] = x.reshape(n, 8, 8, c)
    return xp[:, 1 + dr:9 + dr, 1 + dc:9 + dc].reshape(n, 64, c)


def _fwd(x, w, b):
    n, co = x.shape[0], w.shape[0]
    y = torch.zeros(n, 64, co, dtype=torch.float64) if b is None else b.expand(n, 64, co).clone()
    for t, (dr, dc) in enumerate(TAPS):
        y += _shift(x, dr, dc) @ w[:, :, t // 3, t % 3].t()
    return y


def _dgrad(dy, w):
    dx = torch.zeros(dy.shape[0], 64, w.shape[1], dtype=torch.float64)
    for t, (dr, dc) in enumerate(TAPS):
        dx += _shift(dy, -dr, -dc) @ w[:, :, t // 3, t % 3]
    return dx


def _wgrad(dy, x):
    co, ci = dy.shape[2], x.shape[2]
    dw = torch.zeros(co, ci, 3, 3, dtype=torch.float64)
    for t, (dr, dc) in enumerate(TAPS):
        dw[:, :, t // 3, t % 3] = dy.reshape(-1, co).t() @ _shift(x, dr, dc).reshape(-1, ci)
    return dw


def conv_fwd(x16, w16, bias32=None):
    """y64 [n, 64, co] = bias + sum_{t, ci} x[n, p + off(t), ci] w[co, ci, t] (zero padding)."""
    w = _d(w16)
    return _fwd(_d(x16)[..., :w.shape[1]], w, None if bias32 is None else _d(bias32))


def conv_fwd_abs(x16, w16, bias32=None):
    w = _d(w16).abs()
    return _fwd(_d(x16)[..., :w.shape[1]].abs(), w, None if bias32 is None else _d(bias32).abs())


def conv_dgrad(dy16, w16):
    """dx64 [n, 64, ci_real] = sum_{t, co} dy[n, p - off(t), co] w[co, ci, t]."""
    return _dgrad(_d(dy16), _d(w16))


def conv_dgrad_abs(dy16, w16):
    return _dgrad(_d(dy16).abs(), _d(w16).abs())


def conv_wgrad(dy16, x16, ci_real):
    """dw64 [co, ci_real, 3, 3] = sum_{n, p} dy[n, p, co] x[n, p + off(t), ci]."""
    return _wgrad(_d(dy16), _d(x16)[..., :ci_real])


def conv_wgrad_abs(dy16, x16, ci_real):
    return _wgrad(_d(dy16).abs(), _d(x16)[..., :ci_real].abs())


def weight_images(w32, ci):
    """fp32 [co, ci_real, 3, 3] -> the fp16 forward image [co, 9, ci] (channels >= ci_real zero) and the
    flipped data-gradient image [ci, 9, co]: w'[ci][8 - t][co] = w[co][t][ci]."""
    w = _d(w32)
    co, ci_real = w.shape[0], w.shape[1]
    wf = torch.zeros(co, 9, ci, dtype=torch.float64)
    wf[:, :, :ci_real] = w.reshape(co, ci_real, 9).permute(0, 2, 1)
    wt = wf.flip(1).permute(2, 1, 0).contiguous()
    return wf.float().half(), wt.float().half()  # fp32 values: float64 -> fp32 is exact, one rounding


def planes_nhwc(planes, cpad):
    """fp32 [n, 12, 8, 8] -> fp16 [n, 64, cpad], channels >= 12 zero."""
    p = _d(planes)
    n = p.shape[0]
    out = torch.zeros(n, 64, cpad, dtype=torch.float64)
    out[..., :12] = p.reshape(n, 12, 64).permute(0, 2, 1)
    return out.float().half()


# ------------------------------------------------------------------ heads --
def head_fwd(h16, w16, b32):
    """out64 [n, 64, 3] = b[j] + sum_c h[n, p, c] w[j, c]."""
    return _d(h16) @ _d(w16).t() + _d(b32)


def head_fwd_abs(h16, w16, b32):
    return _d(h16).abs() @ _d(w16).abs().t() + _d(b32).abs()


def head_bwd(h16, dout16, w16):
    """(dh64 [n, 64, 512], dw64 [3, 512], db64 [3]) from dout [n, 64, >= 3] (columns past 2 are not read)."""
    d = _d(dout16)[..., :3]
    return d @ _d(w16), torch.einsum("npj,npc->jc", d, _d(h16)), d.sum(dim=(0, 1))


def head_bwd_abs(h16, dout16, w16):
    d = _d(dout16)[..., :3].abs()
    return d @ _d(w16).abs(), torch.einsum("npj,npc->jc", d, _d(h16).abs()), d.sum(dim=(0, 1))


# ---------------------------------------------------------- integer cases --
def _ints(g, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def _exact16(ref64, abs64, what):
    """The preconditions of a bit-for-bit demand: integer terms whose absolute sum stays below 2^24 (fp32
    accumulation in any order, split partials included, is exact), a finite fp16 result; returns the exact
    result rounded once to fp16."""
    assert float(abs64.max()) < 2.0 ** 24, f"{what}: sum of |terms| {float(abs64.max())} reaches 2^24"
    assert bool((ref64 == ref64.round()).all()), f"{what}: reference is not integer-valued"
    assert bool((ref64.abs() <= abs64).all()), f"{what}: |reference| above its absolute sum"
    assert float(ref64.abs().max()) <= F16_MAX, f"{what}: {float(ref64.abs().max())} is not finite in fp16"
    r16 = (ref64 + 0.0).to(torch.float16)  # + 0.0: an exact zero is +0, as a sum that starts from +0 is
    assert bool(torch.isfinite(r16).all())
    # below 2^24 float64 -> fp32 is exact, so the conversion above rounded once whichever way torch takes
    assert torch.equal(r16, ref64.float().half()) and bool((ref64.float().double() == ref64).all()), what
    return r16


def _sum16(a16, b16):
    """autograd's fp16 accumulation, fp16(float(a) + float(b)), on integer values (exact in float64)."""
    s = a16.double() + b16.double()
    return _exact16(s, a16.double().abs() + b16.double().abs(), "fused add")


@functools.lru_cache(maxsize=None)
def int_case(kind, *shape, seed=0):
    """Integer-valued inputs (x, w, dy, h, dout in -2..2, biases in -8..8) and the exact expected outputs.
    kind "conv" (n, ci, co): x16, w32, bias32, add16 -> y16, ya16 (with the fused add);
    kind "dgrad" (n, ci, co), the forward's shape: dy16, w32, add16 -> dx16, dxa16;
    kind "wgrad" (n, ci_real, ci, co): dy16, x16 (channels >= ci_real hold non-zero values no output may
        depend on) -> dw32 (fp16-rounded values);
    kind "head" (n,): h16, w16, b32, dout16 (column 3 non-zero) -> out16, dh16, dw32, db32.
    The tensors are shared between tests: leave them unchanged."""
    g = torch.Generator().manual_seed(1000003 * seed + sum((i + 1) * 7919 * s for i, s in enumerate(shape)))
    c = types.SimpleNamespace(kind=kind, shape=shape)
    if kind == "conv":
        n, ci, co = shape
        c.x16, c.w32 = _ints(g, (n, 64, ci), 2).half(), _ints(g, (co, ci, 3, 3), 2)
        c.bias32, c.add16 = _ints(g, (co,), 8), _ints(g, (n, 64, co), 2).half()
        c.y16 = _exact16(conv_fwd(c.x16, c.w32, c.bias32), conv_fwd_abs(c.x16, c.w32, c.bias32), "conv forward")
        c.ya16 = _sum16(c.y16, c.add16)
    elif kind == "dgrad":
        n, ci, co = shape
        c.dy16, c.w32 = _ints(g, (n, 64, co), 2).half(), _ints(g, (co, ci, 3, 3), 2)
        c.add16 = _ints(g, (n, 64, ci), 2).half()
        c.dx16 = _exact16(conv_dgrad(c.dy16, c.w32), conv_dgrad_abs(c.dy16, c.w32), "conv data gradient")
        c.dxa16 = _sum16(c.dx16, c.add16)
    elif kind == "wgrad":
        n, ci_real, ci, co = shape
        c.dy16, c.x16 = _ints(g, (n, 64, co), 2).half(), _ints(g, (n, 64, ci), 2).half()
        c.dw32 = _exact16(conv_wgrad(c.dy16, c.x16, ci_real), conv_wgrad_abs(c.dy16, c.x16, ci_real),
                          "conv weight gradient").float()
    elif kind == "head":
        (n,) = shape
        c.h16, c.w16 = _ints(g, (n, 64, 512), 2).half(), _ints(g, (3, 512), 2).half()
        c.b32, c.dout16 = _ints(g, (3,), 8), _ints(g, (n, 64, 4), 2).half()
        c.dout16[..., 3] = c.dout16[..., 3].abs() + 1  # never zero, and never read
        c.out16 = _exact16(head_fwd(c.h16, c.w16, c.b32), head_fwd_abs(c.h16, c.w16, c.b32), "head forward")
        ref, ab = head_bwd(c.h16, c.dout16, c.w16), head_bwd_abs(c.h16, c.dout16, c.w16)
        c.dh16 = _exact16(ref[0], ab[0], "head data gradient")
        c.dw32 = _exact16(ref[1], ab[1], "head weight gradient").float()
        c.db32 = _exact16(ref[2], ab[2], "head bias gradient").float()
    else:
        raise ValueError(kind)
    return c


def accum_bound(ref64, abs64, k):
    """|result - ref| allowed to an fp16 result of k terms accumulated in fp32 in any order: one fp16 rounding
    (2^-11 relative, 2^-25 absolute below the normal range) and twice the worst-case accumulation error
    A = k 2^-24 sum |terms|."""
    return 2.0 ** -11 * ref64.abs() + 2.0 ** -25 + 2.0 * k * 2.0 ** -24 * abs64


# -------------------------------------------------------------- BatchNorm --
def eps32(eps):
    """eps as the kernel sees it: a float argument widened to double."""
    return float(torch.tensor(eps, dtype=torch.float32))


def bn_stats(x16, eps):
    """(mean, biased var, invstd) float64 [C] over boards x squares of x [n, 64, C]."""
    x = _d(x16).reshape(-1, x16.shape[-1])
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, 1.0 / torch.sqrt(var + eps32(eps))


def bn_apply64(x16, mean, invstd, gamma, beta, res16, relu):
    """(BN output before rounding, final output) in float64, no intermediate rounding."""
    bn = (_d(x16) - _d(mean)) * _d(invstd) * _d(gamma) + _d(beta)
    y = bn if res16 is None else bn + _d(res16)
    return bn, (torch.relu(y) if relu else y)


def bn_apply32(x16, mean32, invstd32, gamma32, beta32, res16, relu):
    """bn_apply_kernel in fp32, operation for operation: ((x - m) * iv) * ga + be, rounded to fp16, the
    residual added in fp32 and rounded again, ReLU (anything not > 0, NaN included, becomes +0)."""
    f = lambda t: t.detach().to("cpu", torch.float32)
    v = f(x16) - f(mean32)
    v = v * f(invstd32)
    v = v * f(gamma32)
    v = v + f(beta32)
    hv = v.half()
    if res16 is not None:
        hv = (hv.float() + f(res16)).half()
    if relu:
        hv = torch.where(hv.float() > 0, hv, torch.zeros_like(hv))
    return hv


def _masked(dy, y16, relu):
    return torch.where(y16.detach().cpu().float() > 0, dy, torch.zeros_like(dy)) if relu else dy


def bn_sums64(x16, dy16, y16, relu, mean32, invstd32):
    """(sum g, sum g xhat, sum |g|, sum |g xhat|) float64 [C]: g = dy (where y > 0 if relu),
    xhat = (x - mean) * invstd with the fp32 statistics the kernel is given."""
    C = x16.shape[-1]
    g = _masked(_d(dy16), y16, relu).reshape(-1, C)
    gx = g * ((_d(x16).reshape(-1, C) - _d(mean32)) * _d(invstd32))
    return g.sum(0), gx.sum(0), g.abs().sum(0), gx.abs().sum(0)


def bn_backward64(x16, dy16, y16, relu, mean, invstd, gamma):
    """(dx, dres, dgamma, dbeta) of training BatchNorm in float64."""
    rows = x16.numel() // x16.shape[-1]
    sg, sgx, _, _ = bn_sums64(x16, dy16, y16, relu, mean, invstd)
    g = _masked(_d(dy16), y16, relu)
    xh = (_d(x16) - _d(mean)) * _d(invstd)
    return _d(gamma) * _d(invstd) * (g - sg / rows - xh * sgx / rows), g, sgx, sg


def bn_backward32(x16, dy16, y16, relu, mean32, invstd32, gamma32, sg32, sgx32):
    """bn_backward_kernel's (dx16, dres16) in fp32, operation for operation, from the sums the kernel
    itself returned (sg = its dbeta, sgx = its dgamma): inv_m = 1.0f / rows, mg = sg * inv_m,
    mgx = sgx * inv_m, sc = gamma * iv, dx = fp16(((g - mg) - ((x - m) * iv) * mgx) * sc), dres = fp16(g)."""
    f = lambda t: t.detach().to("cpu", torch.float32)
    rows = x16.numel() // x16.shape[-1]
    inv_m = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(rows), dtype=torch.float32)
    m, iv = f(mean32), f(invstd32)
    mg = f(sg32) * inv_m
    mgx = f(sgx32) * inv_m
    sc = f(gamma32) * iv
    gg = _masked(f(dy16), y16, relu)
    xh = f(x16) - m
    xh = xh * iv
    t = gg - mg
    u = xh * mgx
    t = t - u
    t = t * sc
    return t.half(), gg.half()


def bn_sum_bound(ref64, abs64, C, block_rows=256):
    """|sum - ref| allowed to the BatchNorm reductions: a thread adds block_rows / rl rows in fp32, the block
    its rl row lanes, the terms themselves carry up to 4 roundings; the blocks are added in fp64 and the
    result rounded to fp32 once."""
    rl = 256 // (C // 8)
    return 2.0 ** -24 * ref64.abs() + (block_rows / rl + rl + 4) * 2.0 ** -24 * abs64


def bn_case(n, C, mean, std, seed=0):
    """x16 [n, 64, C] ~ N(mean, std). The (7, 128) case also holds one exactly constant channel
    (BN_CONST_CH) and one whose row 0 lies 10 std from the mean (BN_FAR_CH)."""
    g = torch.Generator().manual_seed(seed * 7919 + n * 1009 + C)
    x = (torch.randn(n, 64, C, generator=g) * std + mean).half()
    if (n, C) == (7, 128):
        x[..., BN_CONST_CH] = 0.71875
        # the outlier widens the channel's own std: a of the others' std out gives delta = 10 of the whole
        # channel's when a^2 = 100 / (1 - 101 / rows)
        x[0, 0, BN_FAR_CH] = mean + 10.0 / (1.0 - 101.0 / (n * 64)) ** 0.5 * std
    return x


def bn_stats_bounds(x16, eps):
    """The float64 statistics and what the shifted-sum algorithm (k = row 0's value) may miss them by. With
    delta = (x[0] - mean) / std per channel the sums of (x - k) and (x - k)^2 carry a (mean - k)^2 = delta^2 var
    term that cancels in the variance, so its error grows with delta^2:
      |var - var64| <= 2^-20 (1 + delta^2) var64 (2^-24 mean^2 where var64 is 0),
      |mean - mean64| <= 2^-23 |mean64| + 2^-20 (1 + |delta|) std64."""
    mean, var, invstd = bn_stats(x16, eps)
    std = torch.sqrt(var)
    x0 = _d(x16).reshape(-1, x16.shape[-1])[0]
    delta = torch.where(std > 0, (x0 - mean) / std.clamp_min(1e-300), torch.zeros_like(std))
    bvar = torch.where(var > 0, 2.0 ** -20 * (1 + delta ** 2) * var, 2.0 ** -24 * mean ** 2)
    bmean = 2.0 ** -23 * mean.abs() + 2.0 ** -20 * (1 + delta.abs()) * std
    return types.SimpleNamespace(mean=mean, var=var, invstd=invstd, std=std, delta=delta, bvar=bvar, bmean=bmean)


def bn_stats_ratios(b, mean32, var32, invstd32, eps):
    """Worst error-to-bound ratios (mean, var, invstd) of fp32 statistics against bn_stats_bounds' `b`; invstd
    is held to 2^-23 relative of 1 / sqrt(var + eps) in float64 from the returned fp32 var."""
    m, v, iv = _d(mean32), _d(var32), _d(invstd32)
    rm = float(((m - b.mean).abs() / b.bmean.clamp_min(1e-300)).max())
    dv = (v - b.var).abs()
    rv = float(torch.where(b.bvar > 0, dv / b.bvar.clamp_min(1e-300), torch.where(dv > 0, dv * float("inf"), dv)).max())
    want = 1.0 / torch.sqrt(v + eps32(eps))
    ri = float(((iv - want).abs() / (2.0 ** -23 * want)).max())
    return rm, rv, ri


def bn_stats_emul32(x16, eps, shift=True):
    """The statistics kernels' arithmetic in fp32 on the CPU: 256-row blocks, rl = 256 // (C / 8) row lanes per
    block, a lane adds (x - k) and (x - k)^2 of every rl-th row in row order, the block adds its lanes in
    order, the block partials are combined in float64; k = row 0's value (shift=False: k = 0, the plain
    E[x^2] - E[x]^2). Returns (mean, var, invstd) fp32 [C]."""
    C = x16.shape[-1]
    x = x16.detach().cpu().reshape(-1, C).float()
    rows = x.shape[0]
    rl = 256 // (C // 8)
    blocks, steps = (rows + 255) // 256, (256 + rl - 1) // rl
    k = x[0].clone() if shift else torch.zeros(C)
    d = torch.zeros(blocks * 256, C)
    d[:rows] = x - k  # rows past the end add an exact 0: the sums do not change
    dd = torch.zeros(blocks, steps * rl, C)
    dd[:, :256] = d.reshape(blocks, 256, C)
    dd = dd.reshape(blocks, steps, rl, C)
    s0 = torch.zeros(blocks, rl, C)
    s1 = torch.zeros(blocks, rl, C)
    for s in range(steps):
        v = dd[:, s]
        s0 = s0 + v
        s1 = s1 + v * v
    a = torch.zeros(blocks, C)
    b = torch.zeros(blocks, C)
    for l in range(rl):
        a = a + s0[:, l]
        b = b + s1[:, l]
    a, b = a.double().sum(0), b.double().sum(0)
    dm = a / rows
    var = (b / rows - dm * dm).clamp_min(0.0)
    return (k.double() + dm).float(), var.float(), (1.0 / torch.sqrt(var + eps32(eps))).float()
