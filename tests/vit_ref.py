"""ViT references (TEST INFRASTRUCTURE ONLY): numpy restatements of csrc/vit_ops.hip in the kernels' stated operation order -- the GPU tests compare
bits against them -- and the whole forward composed from them plus the oracle's convolution / exp / tanh / top-k.

Every fmaf chain (the linear layers, q k^T, p v) goes through ora.conv2d, whose contract is exactly that chain from +0 in ascending k followed by
fmaf(acc, 1, shift) + residual; chains padded with zero products keep their bits (acc + 0 * 0 == acc: a chain that starts at +0 never holds -0).
numpy has no fused multiply-add, which is why dm_erf and the GELU / LayerNorm applies are specified with every operation rounded on its own."""
import numpy as np

from oracle import ora

F = np.float32
ERF_T = (7.853861353153693E-5, -8.010193625184903E-4, 5.188327685732524E-3, -2.685381193529856E-2, 1.128358514861418E-1, -3.761262582423300E-1,
         1.128379165726710E+0)
ERFC_P = (2.326819970068386E-2, -1.387039388740657E-1, 3.687424674597105E-1, -5.824733027278666E-1, 6.210004621745983E-1, -4.944515323274145E-1,
          3.404879937665872E-1, -2.741127028184656E-1, 5.638259427386472E-1)
ERFC_R = (-1.047766399936249E+1, 1.297719955372516E+1, -7.495518717768503E+0, 2.921019019210786E+0, -1.015265279202700E+0, 4.218463358204948E-1,
          -2.820767439740514E-1, 5.641895067754075E-1)
MAXLOGF = 88.72283905206835


def _horner(coef, z):
    p = np.full(z.shape, F(coef[0]), np.float32)
    for c in coef[1:]:
        p = p * z + F(c)
    return p


def dm_erf(x):
    """csrc/detmath.h dm_erf, operation by operation."""
    x = np.ascontiguousarray(x, np.float32)
    a = np.abs(x)
    with np.errstate(all="ignore"):
        small = x * _horner(ERF_T, x * x)
        z = -(a * a)
        under = z < F(-MAXLOGF)
        e = ora.map_f32(np.where(under | ~(a > F(1.0)), F(0.0), z), 0)
        q = F(1.0) / np.where(a > F(1.0), a, F(1.0))
        w = q * q
        y = (e * q) * np.where(a < F(2.0), _horner(ERFC_P, w), _horner(ERFC_R, w))
        r = F(1.0) - np.where(under, F(0.0), y)
        out = np.where(a > F(1.0), np.where(x < F(0.0), -r, r), small)
    assert out.dtype == np.float32
    return out


def erf_sweep():
    """The erf / GELU sweep of the CPU and GPU tests: +-0, the |x| = 1 and 2 branch points and their neighbours, subnormals, the erfc underflow near
    9.4, huge values, a dense grid and random values over 45 decades."""
    rng = np.random.default_rng(5)
    pts = [0.0, -0.0, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0)), 2.0, -2.0,
           np.nextafter(np.float32(2), np.float32(0)), 1e-45, -1e-45, 1e-40, 1.1754944e-38, 9.0, 9.4, 9.5, 10.0, -10.0, 30.0, 1e10, -1e10, 3.0e38]
    return np.concatenate([np.asarray(pts, np.float32), np.linspace(-6, 6, 4001).astype(np.float32), (rng.standard_normal(2000) * 2).astype(np.float32),
                           (10.0 ** rng.uniform(-44, 1, 1000)).astype(np.float32)])


def gelu(x, gelu_tanh=False):
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(all="ignore"):
        if gelu_tanh:
            x3 = (x * x) * x
            t = ora.map_f32(F(0.7978845608028654) * (x + F(0.044715) * x3), 2)
        else:
            t = dm_erf(x * F(0.7071067811865476))
        y = (F(0.5) * x) * (F(1.0) + t)
    assert y.dtype == np.float32
    return y


def _tree64(lane):
    """[..., 64] -> [...]: s[l] += s[l + off] for off = 32 .. 1"""
    off = 32
    while off >= 1:
        lane = lane[..., :off] + lane[..., off:2 * off]
        off //= 2
    return lane[..., 0]


def layer_norm(x, gamma, beta, eps=1e-6):
    """x [rows, D] -> [rows, D] in vit_layer_norm_kernel's order."""
    x = np.ascontiguousarray(x, np.float32)
    R, D = x.shape
    assert D % 4 == 0 and D <= 2048
    k = -(-(D // 4) // 64)
    with np.errstate(all="ignore"):
        d = x - x[:, :1]
        dd = np.zeros((R, k * 256), np.float32)
        dd[:, :D] = d
        dd = dd.reshape(R, k, 64, 4)
        s1 = np.zeros((R, 64), np.float32)
        s2 = np.zeros((R, 64), np.float32)
        for kk in range(k):
            for j in range(4):
                v = dd[:, kk, :, j]
                s1 = s1 + v
                s2 = s2 + v * v
        S1, S2 = _tree64(s1.astype(np.float64)), _tree64(s2.astype(np.float64))
        md = S1 / np.float64(D)
        var = S2 / np.float64(D) - md * md
        var = np.where(var > 0.0, var, 0.0)
        m = md.astype(np.float32)[:, None]
        rstd = (1.0 / np.sqrt(var + np.float64(np.float32(eps)))).astype(np.float32)[:, None]
        y = ((d - m) * rstd) * np.asarray(gamma, np.float32) + np.asarray(beta, np.float32)
    assert y.dtype == np.float32
    return y


U = 2.0 ** -24
TINY = 2.0 ** -149


def ln_bound(x, gamma, beta, eps):
    """tests/groupnorm_ref.py's derivation on one row: k = the longest per-lane chain (4 floats per slot, ceil(D / 256) slots)."""
    x64 = np.asarray(x, np.float64)
    D = x64.shape[1]
    k = 4 * -(-(D // 4) // 64)
    d = x64 - x64[:, :1]
    md = d.mean(1, keepdims=True); mabs = np.abs(d).mean(1, keepdims=True); m2 = (d * d).mean(1, keepdims=True)
    var = np.maximum(m2 - md * md, 0.0)
    s = np.sqrt(var + float(np.float32(eps)))
    A = (k + 1) * mabs + np.abs(md)
    V = (k + 3) * m2 + 2 * np.abs(md) * (k + 1) * mabs
    t = d - md
    ga = np.abs(np.asarray(gamma, np.float64))
    y0 = t / s * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return 1.05 * U * (ga / s * (np.abs(d) + A + np.abs(t)) + ga * np.abs(t) / s * (V / (2 * s * s) + 3) + 2 * np.abs(y0)) + TINY


def layer_norm_float64(x, gamma, beta, eps):
    """torch's LayerNorm in float64 on the fp32 inputs (eps rounded to fp32 first, as the kernel receives it)."""
    import torch
    D = x.shape[-1]
    return torch.nn.functional.layer_norm(torch.from_numpy(np.asarray(x, np.float64)), (D,), torch.from_numpy(np.asarray(gamma, np.float64)),
                                          torch.from_numpy(np.asarray(beta, np.float64)), float(np.float32(eps))).numpy()


def attention_bound(qkv, heads):
    """qkv [N, T, 3 * heads * 64] -> (softmax(q k^T / 8) v in float64 [N, T, heads * 64], the bound on an fp32 result in the kernel's order).

    s: a 64-term fmaf chain, |ds| <= 64 u S with S = sum |q k| / 8.  e = exp(s - m): the subtraction u |s - m|, the argument error 2 * 64 u S through
    exp (relative), dm_exp 2 u.  l: chains of T / 4 terms and two folds.  p = e / l: u.  o: a T-term chain over p v, |do| <= T u sum p |v|.  e's
    relative error E = 128 u S + u R + 2 u (R = max |s - m|) enters p through the numerator and, with the other sign, through l: 2 E.  In all
    |do| <= sum_j p_ij |v_jd| * u * (T + T / 4 + 2 + 1 + 2 * (128 S + R + 2)), times 1.05 for the second-order terms."""
    import torch
    qkv = np.ascontiguousarray(qkv, np.float32)
    N, T, _ = qkv.shape
    t = torch.from_numpy(qkv.astype(np.float64)).reshape(N, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    s = q @ k.transpose(-1, -2) / 8
    p = torch.softmax(s, -1)
    want = (p @ v).permute(0, 2, 1, 3).reshape(N, T, heads * 64).numpy()
    S = (q.abs() @ k.abs().transpose(-1, -2) / 8).amax(-1, keepdim=True)
    R = (s.amax(-1, keepdim=True) - s.amin(-1, keepdim=True))
    bound = (p @ v.abs()) * U * (T + T / 4 + 3 + 2 * (128 * S + R + 2)) * 1.05
    return want, bound.permute(0, 2, 1, 3).reshape(N, T, heads * 64).numpy() + TINY


def _pad32(a, axis):
    n = a.shape[axis]
    pad = [(0, 0)] * a.ndim
    pad[axis] = (0, -n % 32)
    return np.pad(a, pad)


def attention_head(q, k, v):
    """q, k, v [T, 64] of one (image, head) -> (p [T, T], o [T, 64]) in vit_attention_kernel's order."""
    T = q.shape[0]
    with np.errstate(all="ignore"):
        s = ora.conv2d(q.reshape(1, T, 1, 64), k.reshape(T, 1, 1, 64)).reshape(T, T) * F(0.125)
        m = s.max(axis=1, keepdims=True)
        e = ora.map_f32(s - m, 0)
        ep = np.zeros((T, -(-T // 4) * 4), np.float32)
        ep[:, :T] = e
        ep = ep.reshape(T, -1, 4)
        c = np.zeros((T, 4), np.float32)
        for i in range(ep.shape[1]):          # lane r of a row chains keys r, r + 4, ...
            c = c + ep[:, i]
        l = (c[:, 0] + c[:, 1]) + (c[:, 2] + c[:, 3])
        p = e / l[:, None]
        pp = _pad32(p, 1)
        vt = _pad32(np.ascontiguousarray(v.T), 1)
        o = ora.conv2d(pp.reshape(1, T, 1, -1), vt.reshape(64, 1, 1, -1)).reshape(T, 64)
    assert p.dtype == np.float32
    return p, o


def attention(qkv, heads):
    """qkv [N, T, 3 * heads * 64] -> [N, T, heads * 64]"""
    qkv = np.ascontiguousarray(qkv, np.float32)
    N, T, _ = qkv.shape
    D = heads * 64
    out = np.empty((N, T, D), np.float32)
    for n in range(N):
        for h in range(heads):
            sl = [np.ascontiguousarray(qkv[n, :, w * D + h * 64:w * D + h * 64 + 64]) for w in range(3)]
            out[n, :, h * 64:h * 64 + 64] = attention_head(*sl)[1]
    return out


def patchify(x, P):
    x = np.ascontiguousarray(x, np.float32)
    N, H, W, c = x.shape
    return np.ascontiguousarray(x.reshape(N, H // P, P, W // P, P, c).transpose(0, 1, 3, 2, 4, 5)).reshape(N, H // P, W // P, P * P * c)


def class_softmax(x):
    x = np.ascontiguousarray(x, np.float32)
    R, n = x.shape
    with np.errstate(all="ignore"):
        e = ora.map_f32(x - x.max(axis=1, keepdims=True), 0)
        ep = np.zeros((R, -(-n // 64) * 64), np.float32)
        ep[:, :n] = e
        ep = ep.reshape(R, -1, 64)
        lane = np.zeros((R, 64), np.float32)
        for i in range(ep.shape[1]):
            lane = lane + ep[:, i]
        p = e / _tree64(lane)[:, None]
    assert p.dtype == np.float32
    return p


def linear(x, wb, residual=None):
    """x [N, T, Cin] through a (w [Cout][1][1][Cin], bias) layer, + residual [N, T, Cout]"""
    w, b = wb
    N, T, C = x.shape
    r = None if residual is None else residual.reshape(N, T, 1, -1)
    return ora.conv2d(x.reshape(N, T, 1, C), w, shift=b, residual=r).reshape(N, T, -1)


def block(x, convs, tensors, i, cfg):
    """One pre-LN block on x [N, T, D] -> dict(qkv, attn, mlp, x)"""
    N, T, D = x.shape
    b = "blocks.%d." % i
    ln = layer_norm(x.reshape(-1, D), tensors[b + "norm1.weight"], tensors[b + "norm1.bias"], cfg.ln_eps).reshape(N, T, D)
    qkv = linear(ln, convs[b + "attn.qkv"])
    attn = attention(qkv, cfg.heads)
    x1 = linear(attn, convs[b + "attn.proj"], x)
    ln = layer_norm(x1.reshape(-1, D), tensors[b + "norm2.weight"], tensors[b + "norm2.bias"], cfg.ln_eps).reshape(N, T, D)
    mlp = gelu(linear(ln, convs[b + "mlp.fc1"]), cfg.gelu_tanh)
    return dict(qkv=qkv, attn=attn, mlp=mlp, x=linear(mlp, convs[b + "mlp.fc2"], x1))


def embed(convs, tensors, cfg, images):
    """images [N, H, W, 3] -> tokens [N, T, D]"""
    pt = patchify(images, cfg.patch)
    N, gh, gw, _ = pt.shape
    D = cfg.dim
    w, b = convs["patch_embed.proj"]
    pos = np.ascontiguousarray(np.broadcast_to(tensors["vit.pos_rows"].reshape(1, gh, gw, D), (N, gh, gw, D)))
    emb = ora.conv2d(pt, w, shift=b, residual=pos).reshape(N, gh * gw, D)
    cls = np.broadcast_to(tensors["vit.cls_row"].reshape(1, 1, D), (N, 1, D))
    return np.ascontiguousarray(np.concatenate([cls, emb], axis=1), np.float32)


def head(x, convs, tensors, cfg):
    """final tokens [N, T, D] -> (logits, prob, top-k values [N, k], top-k indices [N, k])"""
    cn = layer_norm(np.ascontiguousarray(x[:, 0]), tensors["norm.weight"], tensors["norm.bias"], cfg.ln_eps)
    logits = linear(cn[:, None, :], convs["head"])[:, 0]
    prob = class_softmax(logits)
    tk = [ora.topk(prob[n], cfg.topk) for n in range(len(prob))]
    return logits, prob, np.stack([t[0] for t in tk]), np.stack([t[1] for t in tk])


def forward(sd, cfg, images):
    """The whole model.  -> dict(tokens, blocks [dict per block], logits, prob, topk_val, topk_idx)"""
    from isegmi.vit import vit_layers
    images = np.ascontiguousarray(images, np.float32)
    convs, tensors = vit_layers(sd, cfg, images.shape[1], images.shape[2])
    x = tokens = embed(convs, tensors, cfg, images)
    blocks = []
    for i in range(cfg.depth):
        blocks.append(block(x, convs, tensors, i, cfg))
        x = blocks[-1]["x"]
    logits, prob, tv, ti = head(x, convs, tensors, cfg)
    return dict(tokens=tokens, blocks=blocks, logits=logits, prob=prob, topk_val=tv, topk_idx=ti)
