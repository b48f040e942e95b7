"""CPU restatement of Pose2Seg inference: the five pose-specific stages in numpy, written to the operation order of
csrc/pose2seg_ops.hip, and the whole forward composed from the oracle's conv2d / maxpool / upsample_nearest2x_add / resize_bilinear /
softmax / map_f32.  Test infrastructure only: the product package never imports it."""
import numpy as np

from oracle import ora

S_IN, S_FEAT, S_ALIGN = 512, 128, 64
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
LIMBS = [[16, 14], [14, 12], [17, 15], [15, 13], [12, 13], [6, 12], [7, 13], [6, 7], [6, 8], [7, 9], [8, 10], [9, 11], [2, 3], [1, 2], [1, 3],
         [2, 4], [3, 5], [4, 6], [5, 7]]   # COCO person skeleton, 1-based
F32 = np.float32


# ---------------------------------------------------------------- matrices (fp64, every sum left to right)
def m1_of(h, w):
    s = min(512.0 / w, 512.0 / h)
    return [s, 0.0, 256.0 - s * w / 2.0, 0.0, s, 256.0 - s * h / 2.0]


def m1_inverse(m1):
    s, tx, ty = m1[0], m1[2], m1[5]
    return [1.0 / s, 0.0, -tx / s, 0.0, 1.0 / s, -ty / s]


def mat3(m6):
    return [m6[0], m6[1], m6[2], m6[3], m6[4], m6[5], 0.0, 0.0, 1.0]


def mat3_mul(a, b):
    return [(a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j]) + a[i * 3 + 2] * b[6 + j] for i in range(3) for j in range(3)]


def mat3_adj(m):
    c00 = m[4] * m[8] - m[5] * m[7]; c01 = m[5] * m[6] - m[3] * m[8]; c02 = m[3] * m[7] - m[4] * m[6]
    c10 = m[2] * m[7] - m[1] * m[8]; c11 = m[0] * m[8] - m[2] * m[6]; c12 = m[1] * m[6] - m[0] * m[7]
    c20 = m[1] * m[5] - m[2] * m[4]; c21 = m[2] * m[3] - m[0] * m[5]; c22 = m[0] * m[4] - m[1] * m[3]
    return [c00, c10, c20, c01, c11, c21, c02, c12, c22], (m[0] * c00 + m[1] * c01) + m[2] * c02


# ---------------------------------------------------------------- the one bilinear helper (zero padding, integer pixel centres)
def bilinear(img, sx, sy):
    """img [H, W, C] fp32, sx / sy fp32 arrays of one shape -> [..., C]"""
    img = np.asarray(img, F32)
    H, W = img.shape[:2]
    sx = np.asarray(sx, F32); sy = np.asarray(sy, F32)
    anyt = (sx > -1) & (sx < W) & (sy > -1) & (sy < H)
    fx = np.where(anyt, np.floor(np.where(anyt, sx, 0)), 0).astype(F32)
    fy = np.where(anyt, np.floor(np.where(anyt, sy, 0)), 0).astype(F32)
    x0 = fx.astype(np.int64); y0 = fy.astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        wx1 = (sx - fx).astype(F32); wx0 = (F32(1) - wx1).astype(F32)
        wy1 = (sy - fy).astype(F32); wy0 = (F32(1) - wy1).astype(F32)

    def tap(yy, xx):
        ok = anyt & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        return np.where(ok[..., None], v, F32(0))

    v00, v01, v10, v11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    e = lambda a: a[..., None]
    with np.errstate(invalid="ignore", over="ignore"):
        out = ((v00 * e(wx0) + v01 * e(wx1)) * e(wy0)) + ((v10 * e(wx0) + v11 * e(wx1)) * e(wy1))
    return np.where(anyt[..., None], out, F32(0)).astype(F32)


def _grid(n):
    y, x = np.meshgrid(np.arange(n, dtype=F32), np.arange(n, dtype=F32), indexing="ij")
    return x, y


def warp_coords(m6_f32, x, y):
    m = np.asarray(m6_f32, F32)
    return (m[0] * x + m[1] * y) + m[2], (m[3] * x + m[4] * y) + m[5]


# ---------------------------------------------------------------- 1. letterbox
def letterbox(img_u8, swap_rb=0, round_u8=1, S=S_IN):
    """[h, w, 3] uint8 -> the normalised stem input [S, S, 4]"""
    h, w = img_u8.shape[:2]
    minv = np.asarray(m1_inverse(m1_of(h, w)), F32)
    x, y = _grid(S)
    sx, sy = warp_coords(minv, x, y)
    v = bilinear(img_u8.astype(F32), sx, sy)
    if swap_rb:
        v = v[..., ::-1]
    if round_u8:
        v = np.clip(np.floor(v + F32(0.5)), F32(0), F32(255)).astype(F32)
    out = np.zeros((S, S, 4), F32)
    for c in range(3):
        out[..., c] = (v[..., c] / F32(255) - F32(MEAN[c])) / F32(STD[c])
    return out


# ---------------------------------------------------------------- 2. pose template fit
def fit(kpts, m1, templates, align_corners=0):
    """kpts [17, 3] image pixels (any float dtype: coordinates are taken as fp64), m1 six floats, templates [T, 17, 3] ->
    dict(m3 [6] fp64, err, t (-1: fallback), G / mmask [6] fp32, kalign [17, 3] fp32)"""
    m2 = [0.25, 0.0, 0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 1.0]
    m21 = mat3_mul(m2, mat3(m1))
    kx = [(m21[0] * float(p[0]) + m21[1] * float(p[1])) + m21[2] for p in kpts]
    ky = [(m21[3] * float(p[0]) + m21[4] * float(p[1])) + m21[5] for p in kpts]
    v = [F32(p[2]) if np.isfinite(p[0]) and np.isfinite(p[1]) else F32(0) for p in kpts]   # a non-finite coordinate counts as not visible
    tp = np.asarray(templates, F32)
    best, best_err, best_A = -1, 0.0, None
    for t in range(tp.shape[0]):
        S = [0.0] * 9; B = [0.0] * 6; wsum = 0.0; n = 0
        used = [j for j in range(17) if v[j] > 0 and float(tp[t, j, 2]) > 0.0]
        for j in used:
            w = float(tp[t, j, 2]); p = (kx[j], ky[j], 1.0); qx, qy = float(tp[t, j, 0]), float(tp[t, j, 1])
            for a in range(3):
                wp = w * p[a]
                for c in range(3):
                    S[a * 3 + c] = S[a * 3 + c] + wp * p[c]
                B[a * 2] = B[a * 2] + wp * qx
                B[a * 2 + 1] = B[a * 2 + 1] + wp * qy
            wsum = wsum + w; n += 1
        adj, det = mat3_adj(S)
        tr = (S[0] + S[4]) + S[8]
        if not (n >= 3 and abs(det) > 1e-9 * tr * tr * tr):
            continue
        A = [0.0] * 6
        for i in range(3):
            for k in range(2):
                A[k * 3 + i] = ((adj[i * 3] * B[k] + adj[i * 3 + 1] * B[2 + k]) + adj[i * 3 + 2] * B[4 + k]) / det
        err = 0.0
        for j in used:
            w = float(tp[t, j, 2])
            rx = ((A[0] * kx[j] + A[1] * ky[j]) + A[2]) - float(tp[t, j, 0])
            ry = ((A[3] * kx[j] + A[4] * ky[j]) + A[5]) - float(tp[t, j, 1])
            err = err + w * (rx * rx + ry * ry)
        err = err / wsum
        if err != err:
            continue
        if best < 0 or err < best_err:
            best, best_err, best_A = t, err, A
    if best >= 0:
        H = best_A + [0.0, 0.0, 1.0]
        err = best_err
    else:
        err = 0.0
        vis = [j for j in range(17) if v[j] > 0]
        if not vis:
            H = [0.5, 0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 1.0]
        else:
            x0 = x1 = kx[vis[0]]; y0 = y1 = ky[vis[0]]
            for j in vis[1:]:
                x0 = min(x0, kx[j]); x1 = max(x1, kx[j]); y0 = min(y0, ky[j]); y1 = max(y1, ky[j])
            side = max(x1 - x0, y1 - y0) * 1.2
            if side < 8.0:
                side = 8.0
            k = 64.0 / side
            cx = (x0 + x1) * 0.5; cy = (y0 + y1) * 0.5
            H = [k, 0.0, 32.0 - k * cx, 0.0, k, 32.0 - k * cy, 0.0, 0.0, 1.0]
    G = align_matrix(H, align_corners)
    Mm = mat3_mul(H, m21)
    kal = np.array([[(H[0] * kx[j] + H[1] * ky[j]) + H[2], (H[3] * kx[j] + H[4] * ky[j]) + H[5], 0.0] for j in range(17)]).astype(F32)
    kal[:, 2] = v
    return dict(m3=np.array(H[:6]), err=err, t=best, G=np.array(G[:6]).astype(F32), mmask=np.array(Mm[:6]).astype(F32), kalign=kal)


def align_matrix(H, align_corners):
    """upstream's theta = inv(A H A^-1) with A = [[2/128, 0, -1], [0, 2/128, -1]], folded with affine_grid's normalise and grid_sample's
    unnormalise over a 128 x 128 grid into one pixel-space matrix (fp64)"""
    An = [2.0 / 128.0, 0.0, -1.0, 0.0, 2.0 / 128.0, -1.0, 0.0, 0.0, 1.0]
    Ai = [64.0, 0.0, 64.0, 0.0, 64.0, 64.0, 0.0, 0.0, 1.0]
    M = mat3_mul(mat3_mul(An, list(H)), Ai)
    adj, dM = mat3_adj(M)
    theta = [a / dM for a in adj]
    nsc = 2.0 / 127.0 if align_corners else 2.0 / 128.0
    nof = -1.0 if align_corners else 1.0 / 128.0 - 1.0
    usc = 63.5 if align_corners else 64.0
    Nrm = [nsc, 0.0, nof, 0.0, nsc, nof, 0.0, 0.0, 1.0]
    Un = [usc, 0.0, 63.5, 0.0, usc, 63.5, 0.0, 0.0, 1.0]
    return mat3_mul(Un, mat3_mul(theta, Nrm))


# ---------------------------------------------------------------- 3. Affine-Align
def affine_align(feat, G):
    """feat [Hf, Wf, C] -> [64, 64, C]"""
    x, y = _grid(S_ALIGN)
    sx, sy = warp_coords(G, x, y)
    return bilinear(feat, sx, sy)


# ---------------------------------------------------------------- 4. skeleton features
def skeleton(kal):
    """kal [17, 3] align-frame keypoints -> [64, 64, 55]"""
    kal = np.asarray(kal, F32)
    x, y = _grid(S_ALIGN)
    out = np.zeros((S_ALIGN, S_ALIGN, 55), F32)
    for j in range(17):
        if not kal[j, 2] > 0:
            continue
        dx = x - kal[j, 0]; dy = y - kal[j, 1]
        d2 = dx * dx + dy * dy
        e = ((d2 * F32(0.5)) / F32(3)) / F32(3)
        out[..., j] = np.where(e <= F32(4.6052), ora.map_f32(-e, 0), F32(0))
    for l, (a, b) in enumerate(LIMBS):
        a -= 1; b -= 1
        if not (kal[a, 2] > 0 and kal[b, 2] > 0):
            continue
        ax, ay, bx, by = kal[a, 0], kal[a, 1], kal[b, 0], kal[b, 1]
        lx = bx - ax; ly = by - ay
        norm = np.sqrt(lx * lx + ly * ly)
        if not norm > 0:
            continue
        ux = lx / norm; uy = ly / norm
        x_lo = max(np.rint(min(ax, bx) - F32(1)), F32(0)); x_hi = min(np.rint(max(ax, bx) + F32(1)), F32(64))
        y_lo = max(np.rint(min(ay, by) - F32(1)), F32(0)); y_hi = min(np.rint(max(ay, by) + F32(1)), F32(64))
        inside = (x >= x_lo) & (x < x_hi) & (y >= y_lo) & (y < y_hi)
        perp = (x - ax) * uy - (y - ay) * ux
        on = inside & (np.abs(perp) < F32(1))
        out[..., 17 + 2 * l] = np.where(on, ux, F32(0))
        out[..., 18 + 2 * l] = np.where(on, uy, F32(0))
    return out


# ---------------------------------------------------------------- 5. softmax + reverse warp
def mask_prob(logits):
    return ora.softmax(logits)[..., 1]


def reverse_warp(logits, mmask, h, w):
    """logits [64, 64, 2] -> (mask u8 [h, w], box xyxy fp32 (right / bottom exclusive; zeros when empty))"""
    p = mask_prob(logits)
    y, x = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
    sx, sy = warp_coords(mmask, x, y)
    m = (bilinear(p[..., None], sx, sy)[..., 0] > F32(0.5)).astype(np.uint8)
    ys, xs = np.nonzero(m)
    box = np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], F32) if len(xs) else np.zeros(4, F32)
    return m, box


# ---------------------------------------------------------------- weights, restated from the state dict
def _krsc(w):
    return np.ascontiguousarray(np.asarray(w, F32).transpose(0, 2, 3, 1))


def _fold_bn(sd, p, eps=1e-5):
    """nn.BatchNorm2d in eval: y = (x - mean) / sqrt(var + eps) * weight + bias = x * scale + shift"""
    scale = (np.asarray(sd[p + ".weight"], F32) / np.sqrt(np.asarray(sd[p + ".running_var"], F32) + F32(eps))).astype(F32)
    return scale, (np.asarray(sd[p + ".bias"], F32) - np.asarray(sd[p + ".running_mean"], F32) * scale).astype(F32)


def _pad_cin(w, cin):
    return np.concatenate([w, np.zeros(w.shape[:3] + (cin - w.shape[3],), F32)], 3) if w.shape[3] < cin else w


def params_from_state_dict(sd, cat_skeleton=True):
    """the forward's parameters straight from the state dict (weights.pose2seg_state_dict names): KRSC weights, BN folded, the stem's input
    padded to 4 channels, segnet.conv1's to the RoI tensor's (C + 64 with the skeleton)"""
    def cbn(name, bn):
        return (_krsc(sd[name + ".weight"]),) + _fold_bn(sd, bn)

    def bneck(nm, stride):
        p = dict(conv1=cbn(nm + ".conv1", nm + ".bn1"), conv2=cbn(nm + ".conv2", nm + ".bn2"), conv3=cbn(nm + ".conv3", nm + ".bn3"), stride=stride)
        if nm + ".downsample.0.weight" in sd:
            p["down"] = cbn(nm + ".downsample.0", nm + ".downsample.1")
        return p

    def blocks(prefix):
        return sorted({int(k[len(prefix):].split(".")[0]) for k in sd if k.startswith(prefix)})

    st = cbn("backbone.conv1", "backbone.bn1")
    stem = (_pad_cin(st[0], 4),) + st[1:]
    stages = [[bneck("backbone.layers.%d.%d" % (l, b), 2 if (l > 0 and b == 0) else 1) for b in blocks("backbone.layers.%d." % l)] for l in range(4)]
    lateral = [(_krsc(sd["fpn.lateral%d.weight" % l]), np.asarray(sd["fpn.lateral%d.bias" % l], F32)) for l in (2, 3, 4, 5)]
    p2_out = (_krsc(sd["fpn.output2.weight"]), np.asarray(sd["fpn.output2.bias"], F32))
    C = p2_out[0].shape[0]
    c1 = cbn("segnet.conv1", "segnet.bn1")
    seg = dict(conv1=(_pad_cin(c1[0], C + 64 if cat_skeleton else C),) + c1[1:],
               stage1=[bneck("segnet.stage1.%d" % b, 1) for b in blocks("segnet.stage1.")],
               stage2=[bneck("segnet.stage2.%d" % b, 1) for b in blocks("segnet.stage2.")],
               out=(_krsc(sd["segnet.conv_out.weight"]), np.asarray(sd["segnet.conv_out.bias"], F32)))
    return dict(stem=stem, stages=stages, lateral=lateral, p2_out=p2_out, seg=seg, templates=np.asarray(sd["pose_templates"], F32))


# ---------------------------------------------------------------- the whole forward
def _bottleneck(x, p, stride):
    t = ora.conv2d(x, p["conv1"][0], 1, 0, p["conv1"][1], p["conv1"][2], act=1)
    t = ora.conv2d(t, p["conv2"][0], stride, 1, p["conv2"][1], p["conv2"][2], act=1)
    sc = x if "down" not in p else ora.conv2d(x, p["down"][0], stride, 0, p["down"][1], p["down"][2])
    return ora.conv2d(t, p["conv3"][0], 1, 0, p["conv3"][1], p["conv3"][2], residual=sc, act=1)


def forward(sd, images, kpts, cfg):
    """sd: the state dict; images: list of [h, w, 3] uint8; kpts: list of [n_i, 17, 3]; cfg: a Pose2SegConfig
    -> dict(p2 [N, 128, 128, C], roi [R, 64, 64, Croi], logits [R, 64, 64, 2], masks / boxes per image)"""
    params = params_from_state_dict(sd, bool(cfg.cat_skeleton))
    x = np.stack([letterbox(im, cfg.swap_rb, cfg.warp_round_u8) for im in images])
    st = params["stem"]
    x = ora.maxpool(ora.conv2d(x, st[0], 2, 3, st[1], st[2], act=1), 3, 2, 1)
    feats = []
    for stage in params["stages"]:
        for b, p in enumerate(stage):
            x = _bottleneck(x, p, p["stride"])
        feats.append(x)
    lat = params["lateral"]
    inner = ora.conv2d(feats[3], lat[3][0], 1, 0, None, lat[3][1])
    for l in (2, 1, 0):
        lt = ora.conv2d(feats[l], lat[l][0], 1, 0, None, lat[l][1])
        inner = (ora.upsample_nearest2x_add(inner, lt) if cfg.fpn_upsample == "nearest"
                 else ora.resize_bilinear(inner, lt.shape[1], lt.shape[2], add=lt))
    p2 = ora.conv2d(inner, params["p2_out"][0], 1, 1, None, params["p2_out"][1])
    C = p2.shape[3]
    croi = C + 64 if cfg.cat_skeleton else C
    rois, fits, owner = [], [], []
    for n, (im, kp) in enumerate(zip(images, kpts)):
        m1 = m1_of(*im.shape[:2])
        for k in np.asarray(kp, F32).reshape(-1, 17, 3):
            f = fit(k, m1, params["templates"], cfg.align_corners)
            r = np.zeros((S_ALIGN, S_ALIGN, croi), F32)
            r[..., :C] = affine_align(p2[n], f["G"])
            if cfg.cat_skeleton:
                r[..., C:C + 55] = skeleton(f["kalign"])
            rois.append(r); fits.append(f); owner.append(n)
    out = dict(p2=p2, fits=fits, masks=[], boxes=[])
    if rois:
        sg = params["seg"]
        t = ora.conv2d(np.stack(rois), sg["conv1"][0], 2, 3, sg["conv1"][1], sg["conv1"][2], act=1)
        for p in sg["stage1"]:
            t = _bottleneck(t, p, 1)
        t = ora.resize_bilinear(t, 2 * t.shape[1], 2 * t.shape[2])
        for p in sg["stage2"]:
            t = _bottleneck(t, p, 1)
        logits = ora.conv2d(t, sg["out"][0], 1, 0, None, sg["out"][1])
        out["roi"] = np.stack(rois)
    else:
        logits = np.zeros((0, S_ALIGN, S_ALIGN, 2), F32)
        out["roi"] = np.zeros((0, S_ALIGN, S_ALIGN, croi), F32)
    out["logits"] = logits
    for n, im in enumerate(images):
        ms, bs = [], []
        for r in [i for i, o in enumerate(owner) if o == n]:
            m, b = reverse_warp(logits[r], fits[r]["mmask"], *im.shape[:2])
            ms.append(m); bs.append(b)
        out["masks"].append(ms); out["boxes"].append(bs)
    return out
