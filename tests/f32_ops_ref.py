"""References, inputs and case lists shared by tests/test_gpu_f32_ops.py (GPU) and tests/test_f32_ops_cpu.py (no GPU): plain torch on the
CPU, float64 unless a dtype is passed.  Nothing here touches the HIP library."""
import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------------------------------------------- conv / GEMM
def w_to_torch(w):
    """[groups][taps][M][K] (the hooks' layout) -> torch's [groups * M][K][k][k]."""
    g_, taps, M, K = w.shape
    k = 3 if taps == 9 else 1
    return w.reshape(g_, k, k, M, K).permute(0, 3, 4, 1, 2).reshape(g_ * M, K, k, k)


def conv_ref(x, w, scale=None, shift=None, res=None, stride=1, relu=False, dtype=torch.float64):
    """NHWC conv (3x3 zero padding 1 / 1x1) with the hooks' epilogue: relu?(scale * conv + shift + res).  x [B,H,H,C], w [g,taps,M,K]."""
    g_, taps = w.shape[0], w.shape[1]
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w_to_torch(w.to(dtype)), stride=stride, padding=1 if taps == 9 else 0, groups=g_).permute(0, 2, 3, 1)
    if scale is not None:
        y = y * scale.to(dtype)
    if shift is not None:
        y = y + shift.to(dtype)
    if res is not None:
        y = y + res.to(dtype)
    return torch.relu(y) if relu else y


def conv_brute(x, w, stride=1):
    """The same sum as explicit loops (tiny shapes only): the check of w_to_torch / conv_ref."""
    B, H, _, _ = x.shape
    g_, taps, M, K = w.shape
    Ho = (H - 1) // stride + 1
    y = torch.zeros(B, Ho, Ho, g_ * M, dtype=torch.float64)
    for g in range(g_):
        for t in range(taps):
            dy, dx = (t // 3 - 1, t % 3 - 1) if taps == 9 else (0, 0)
            for oy in range(Ho):
                for ox in range(Ho):
                    iy, ix = oy * stride + dy, ox * stride + dx
                    if 0 <= iy < H and 0 <= ix < H:
                        y[:, oy, ox, g * M:(g + 1) * M] += x[:, iy, ix, g * K:(g + 1) * K].double() @ w[g, t].double().T
    return y


def unvjp_pack_ref(w):
    """[taps][M][K] -> [taps - 1 - tap][K][M]: the UNet's data-gradient image (same dtype, exact)."""
    return w.flip(0).transpose(1, 2).contiguous()


def cvjp_transpose_ref(w, scale, ldt):
    """[M][K] (* scale[m] in w's dtype) -> [K][ldt] with zero rows beyond M: ResNeXt29's 1x1 data-gradient image."""
    M, K = w.shape
    out = torch.zeros(K, ldt, dtype=w.dtype)
    out[:, :M] = (w * scale[:, None] if scale is not None else w).T
    return out


def cvjp_pack_grouped_ref(w, scale):
    """[g][tap][m][k] * scale[g * G + m] -> [g][8 - tap][k][m]: ResNeXt29's grouped-3x3 data-gradient image."""
    g_, taps, G, _ = w.shape
    return (w * scale.reshape(g_, 1, G, 1)).flip(1).transpose(2, 3).contiguous()


def dilate2x_ref(g):
    B, Ho, _, C = g.shape
    d = torch.zeros(B, 2 * Ho, 2 * Ho, C, dtype=g.dtype)
    d[:, ::2, ::2] = g
    return d


def upsample2x_bwd_ref(g, add=None):
    """2x2 sums in the kernel's order ((a + e) + f) + h (+ add), in g's dtype."""
    v = ((g[:, ::2, ::2] + g[:, ::2, 1::2]) + g[:, 1::2, ::2]) + g[:, 1::2, 1::2]
    return v + add if add is not None else v


def conv_dgrad_ref(g_y, w, H, form=0, stride=1, scale=None, mask_y=None, acc=None):
    """float64 autograd of the forward conv (form 1: interpolate x2 + conv; form 2: conv then * scale, then ReLU'(mask_y) on g_y)."""
    g_, taps, M, K = w.shape
    B = g_y.shape[0]
    x = torch.zeros(B, H, H, g_ * K, dtype=torch.float64, requires_grad=True)
    xin = x.permute(0, 3, 1, 2)
    if form == 1:
        xin = F.interpolate(xin, scale_factor=2, mode='nearest')
    y = F.conv2d(xin, w_to_torch(w.double()), stride=stride, padding=1 if taps == 9 else 0, groups=g_).permute(0, 2, 3, 1)
    if scale is not None:
        y = y * scale.double()
    g = g_y.double()[..., :y.shape[-1]] if g_y.shape[-1] != y.shape[-1] else g_y.double()
    if mask_y is not None:
        g = torch.where(mask_y > 0, g, torch.zeros_like(g))
    gx, = torch.autograd.grad(y, x, g)
    return gx + acc.double() if acc is not None else gx


def gemm_f32_dispatch(N, M, K, taps, groups=1, two=False, slab_floats=0, n_ref=0, ldc=None):
    """The launcher's own rules (csrc/gemm_f32.hip, launch_gemm_f32, plain fp32 path, epi 0) -> dict(bm, narrow, two, splits)."""
    ldc = ldc if ldc is not None else groups * M
    gx, gy128 = -(-N // 128), -(-M // 128)
    small = (not two) and M > 64 and gx * gy128 * max(groups, 1) < 128
    bm = 64 if (M <= 64 or small) else 128
    gy = -(-M // bm)
    nks = taps * (K // 16)
    S = 1
    if groups <= 1 and slab_floats > 0:
        nr = n_ref if n_ref > 0 else N
        wgs_ref = -(-nr // 128) * (1 if M <= 64 else gy128)
        if wgs_ref < 384:
            S = min(768 // wgs_ref, nks // 4)
            while S > 1 and S * nr * ldc > slab_floats:
                S -= 1
            if S < 2 or N > nr:
                S = 1
    z = groups if groups > 1 else S
    narrow = (not two) and bm == 64 and gx * gy * z < 256 and nks >= 8
    return dict(bm=128 if two else bm, narrow=int(narrow), two=int(two), splits=S)


def dispatch_batches(rows_per_sample, M, K, taps, groups=1, two=False, max_rows=20000, extra=()):
    """Batch sizes on both sides of every change of gemm_f32_dispatch(B * rows_per_sample, ...) with B * rows <= max_rows, plus B = 1 and
    `extra`, ascending."""
    bs = {1, *extra}
    prev = gemm_f32_dispatch(rows_per_sample, M, K, taps, groups, two)
    B = 2
    while B * rows_per_sample <= max_rows:
        cur = gemm_f32_dispatch(B * rows_per_sample, M, K, taps, groups, two)
        if cur != prev:
            bs.update((B - 1, B))
        prev = cur
        B += 1
    return sorted(bs)


# B, H, cin, cout, taps, stride, c1 (two-part input), residual, relu, groups — the forms of test_gpu_parity.X3_CASES (split-format
# residual = plain residual here), then this tier's own edges
CONV_CASES = [
    (2, 32, 128, 128, 9, 1, 0, 1, False, 1), (1, 32, 128, 128, 9, 1, 0, 0, False, 1),
    (3, 16, 256, 256, 9, 1, 0, 0, True, 1), (2, 32, 256, 256, 9, 2, 0, 0, False, 1),
    (2, 16, 384, 128, 1, 1, 256, 0, False, 1), (5, 8, 512, 256, 9, 1, 256, 1, False, 1),
    (7, 4, 256, 768, 1, 1, 0, 0, False, 1), (65, 32, 384, 128, 9, 1, 256, 1, False, 1),
    (3, 16, 512, 512, 9, 1, 0, 0, True, 4), (2, 16, 2048, 2048, 9, 2, 0, 0, True, 8), (2, 32, 64, 512, 1, 1, 0, 0, True, 1),
    (3, 8, 1024, 512, 1, 1, 0, 1, True, 1),
    # M tails (the class counts), M = 64 (the 64-row tile on a full grid), N off the 32- and 128-row tiles (5 x 5 and 7 x 7 maps), K = 16
    (3, 8, 256, 10, 1, 1, 0, 0, False, 1), (3, 8, 128, 35, 9, 1, 0, 1, False, 1), (70, 32, 64, 64, 9, 1, 0, 0, True, 1),
    (3, 5, 128, 128, 9, 1, 0, 0, False, 1), (3, 7, 256, 192, 9, 2, 0, 1, False, 1), (2, 16, 16, 128, 9, 1, 0, 0, False, 1),
    (2, 16, 16, 256, 1, 1, 0, 0, False, 1),
]


def conv_inputs(case, B, seed_extra=0):
    """Deterministic operands of a CONV_CASES entry for batch B (the first samples of a larger batch are the smaller batch's)."""
    _, H, cin, cout, taps, stride, c1, with_res, relu, groups = case
    g = torch.Generator().manual_seed(3000 + H + cin + cout + seed_extra)
    Kg, Mg = cin // groups, cout // groups
    w = (torch.rand(groups, taps, Mg, Kg, generator=g) * 2 - 1) * 0.1
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.rand(cout, generator=g) * 2 - 1
    Ho = (H - 1) // stride + 1
    gb = torch.Generator().manual_seed(4000 + H + cin)
    x = torch.rand(B, H, H, cin, generator=gb) * 2 - 1
    res = (torch.rand(B, Ho, Ho, cout, generator=gb) * 2 - 1) if with_res else None
    return x, w, scale, shift, res


# --------------------------------------------------------------------------------------------------------------- GroupNorm
def groupnorm_ref(x, gamma, beta, ss=None, silu=False):
    """GroupNorm32 over [B][HW][C] in x's dtype (+ scale-shift with one [2C] row, + SiLU)."""
    C = x.shape[2]
    y = F.group_norm(x.permute(0, 2, 1), 32, gamma, beta, eps=1e-5).permute(0, 2, 1)
    if ss is not None:
        y = y * (1 + ss[:C]) + ss[C:]
    return F.silu(y) if silu else y


# (HW, C) of every map the UNet normalises (32x32 .. 4x4, 128 .. 384 channels), then the concatenated inputs whose groups straddle the parts
GN_MAPS = [(1024, 128), (256, 128), (256, 256), (64, 256), (16, 256), (1024, 256), (1024, 384), (256, 384), (256, 512), (64, 512), (16, 512)]
GN_CASES = [(hw, c, 0, ss, silu, False) for (hw, c) in GN_MAPS for (ss, silu) in ((False, True), (True, True))] + \
           [(256, 128, 0, False, False, True), (64, 256, 0, True, False, True)] + \
           [(hw, c, 256, ss, silu, add) for (hw, c) in ((256, 384), (1024, 384), (64, 512)) for (ss, silu, add) in ((False, True, True), (True, False, False), (True, True, True))]


def gn_inputs(case, B=3):
    hw, C, c1, with_ss, silu, with_add = case
    g = torch.Generator().manual_seed(5000 + hw + C + c1 + 2 * with_ss + silu)
    x = 3 + 0.5 * torch.randn(B, hw, C, generator=g)                       # a mean far from zero: a one-pass variance would show
    gamma = 1 + 0.3 * torch.randn(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    ss = 0.3 * torch.randn(2 * C, generator=g) if with_ss else None
    gy = torch.randn(B, hw, C, generator=g)
    add = torch.randn(B, hw, C, generator=g) if with_add else None
    add2 = torch.randn(B, hw, C, generator=g) if with_add else None
    return x, gamma, beta, ss, gy, add, add2


def gn_fwd_bwd(x, gamma, beta, ss, silu, gy, dtype):
    xx = x.to(dtype).requires_grad_(True)
    y = groupnorm_ref(xx, gamma.to(dtype), beta.to(dtype), None if ss is None else ss.to(dtype), silu)
    gx, = torch.autograd.grad(y, xx, gy.to(dtype))
    return y.detach(), gx


# --------------------------------------------------------------------------------------------------------------- attention
def attention_ref(qkv, heads):
    """QKVAttention with the head-major channel split (head h: q, k, v = 64 channels each from h * 192) and the 1/8 scale of
    1/sqrt(sqrt(64)) on q and on k; explicit softmax, in qkv's dtype.  qkv [B][T][heads * 192] -> [B][T][heads * 64]."""
    B, T, _ = qkv.shape
    q, k, v = qkv.reshape(B, T, heads, 3, 64).permute(3, 0, 2, 1, 4)          # each [B][heads][T][64]
    s = (q @ k.transpose(-1, -2)) * 0.125
    s = s - s.max(-1, keepdim=True)[0]
    p = s.exp()
    p = p / p.sum(-1, keepdim=True)
    return (p @ v).permute(0, 2, 1, 3).reshape(B, T, heads * 64)


ATT_CASES = [(T, heads, B, spread) for T in (16, 64, 256) for heads in (1, 4) for B in (1, 5) for spread in (False,)] + [(64, 4, 2, True)]


def att_inputs(case):
    T, heads, B, spread = case
    g = torch.Generator().manual_seed(6000 + T + heads + B)
    qkv = torch.randn(B, T, heads * 192, generator=g)
    qkv.view(B, T, heads, 3, 64)[..., 0:2, :] *= 1.5        # logits q.k / 8 ~ N(0, 2.25^2): a softmax neither flat nor one-hot
    if spread:                                              # one query row whose logits spread by ~30: the max subtraction matters
        qkv[0, 3, 0:64] *= 1.5
        qkv[0, 5, 64:128] = qkv[0, 3, 0:64] / 1.5 * 0.85
    go = torch.randn(B, T, heads * 64, generator=g)
    return qkv, go


def att_fwd_bwd(qkv, go, heads, dtype):
    q = qkv.to(dtype).requires_grad_(True)
    o = attention_ref(q, heads)
    gq, = torch.autograd.grad(o, q, go.to(dtype))
    return o.detach(), gq


def split_qkv(t, heads):
    """[B][T][heads * 192] -> (q, k, v) parts [B][T][heads][64]."""
    B, T, _ = t.shape
    r = t.reshape(B, T, heads, 3, 64)
    return r[..., 0, :], r[..., 1, :], r[..., 2, :]


def rel(a, ref):
    return float((a.double() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), 1e-300)


def measure_fp32_cpu_errors():
    """The error of the same ops in fp32 torch on the CPU against float64, on the tests' own inputs: the worst relative error
    (max |err| / max |ref|) of the GroupNorm backward and of the attention backward's dq / dk / dv, over all cases."""
    gn = 0.0
    for case in GN_CASES:
        x, gamma, beta, ss, gy, _, _ = gn_inputs(case)
        _, g64 = gn_fwd_bwd(x, gamma, beta, ss, case[4], gy, torch.float64)
        _, g32 = gn_fwd_bwd(x, gamma, beta, ss, case[4], gy, torch.float32)
        gn = max(gn, rel(g32, g64))
    att = 0.0
    for case in ATT_CASES:
        qkv, go = att_inputs(case)
        _, g64 = att_fwd_bwd(qkv, go, case[1], torch.float64)
        _, g32 = att_fwd_bwd(qkv, go, case[1], torch.float32)
        for a, r in zip(split_qkv(g32, case[1]), split_qkv(g64, case[1])):
            att = max(att, rel(a, r))
    return gn, att


# The measured values (test_f32_ops_cpu.test_fp32_cpu_reference_errors reproduces them) and the bounds derived from them: the kernels sum
# sequentially over up to 256 rows / 12288 elements where torch sums pairwise, at most sqrt(n) / log n ~ 8 more accumulated rounding.
GN_BWD_FP32_CPU_ERR = 8.81e-7
ATT_BWD_FP32_CPU_ERR = 1.14e-6
GN_BWD_TOL = 8 * GN_BWD_FP32_CPU_ERR
ATT_BWD_TOL = 8 * ATT_BWD_FP32_CPU_ERR
F32_TOL = 1e-5            # the bound the project demands of the split-f16 tier as "fp32-grade": the exact tier may not be worse
